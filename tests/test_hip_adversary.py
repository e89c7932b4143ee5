"""The speaker adversary's two launches (dvae_adv_rows, dvae_adv_params; csrc/adversary.hip) on the MI355X
through the C ABI, against the float64 restatement of tests/adv_ref.py.

Every output is held to the bound derived in adv_ref (from 2^-24 and the kernels' summation depths, not from what the kernels
give); the arg-max and the counts are exact; what the contract calls exact — the zeros of an ignored row, the +0.0 of dx under
lambda = 0 whatever the row holds, the padding columns of dw1, two launches — is compared bit for bit.  The seeded inputs keep
every pre-activation and every top-two logit gap ten bounds away from zero (tests/test_adv_ref.py checks that on the CPU), so
no element is left out.  Every buffer a launch may write is a guarded one of tests/kernel_harness.py, pre-filled with 0xFF;
the inputs carry NaN wherever the entry points must not read.  The worst error / bound per case is printed at the module's end.

Worst error / bound on the MI355X over the five cases: h 0.534 (the one-row case), loss 0.026, g2 0.108, g1 0.016, dx 0.008,
dw1 0.017, db1 0.015, dw2 0.059, db2 0.024, out 0.014.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, F32, F64, guards, L, ok, Pad, st, untouched, Worst
import dvae_amd  # noqa: E402,F401
import adv_ref as A  # noqa: E402

WORST = Worst("test_hip_adversary.py (rows: case)")
note = WORST.note
ROW_KEYS = ("h", "loss", "g2", "g1")
GRAD_KEYS = ("dw1", "db1", "dw2", "db2")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


@pytest.fixture(scope="module")
def cases():
    """inputs, float64 results and bounds of every case: computed once, shared, never changed"""
    out = {}
    for name in A.CASES:
        c = A.make_case(name)
        args = (c["x"], c["labels"], c["w1"], c["b1"], c["w2"], c["b2"], c["lam"], c["inv_rows"])
        res = A.rows64(*args)
        out[name] = dict(c, res=res, par=A.params64(c["x"], c["labels"], res, c["inv_rows"]), bnd=A.bounds(*args, res=res))
    return out


class Net:
    """a case on the device: x as the columns col0 .. col0 + D - 1 of a NaN table [R, ldx], w1 padded with NaN columns to
    ldw1 = D rounded up to 4, NaN around everything; the outputs as guarded, poisoned buffers"""

    def __init__(self, c, lam=None, x=None):
        R, D, H, S = c["R"], c["D"], c["H"], c["S"]
        self.dims, self.ldx, self.col0, self.ldw1 = (R, D, H, S), c["ldx"], c["col0"], (D + 3) // 4 * 4
        table = np.full((R, self.ldx), np.nan, F32)
        table[:, self.col0:self.col0 + D] = c["x"] if x is None else x
        w1 = np.full((H, self.ldw1), np.nan, F32)
        w1[:, :D] = c["w1"]
        self.x, self.w1 = Pad(table), Pad(w1, before=4)
        self.b1, self.w2, self.b2 = Pad(c["b1"]), Pad(c["w2"], before=4), Pad(c["b2"])
        self.labels = Buf(data=np.ascontiguousarray(c["labels"], np.int32))
        self.coef = Pad(np.array([c["lam"] if lam is None else lam], F32))
        self.inv_rows = c["inv_rows"]
        self.new_outputs()

    def new_outputs(self, lddx=None, dx_col0=None):
        R, D, H, S = self.dims
        self.lddx = self.ldx if lddx is None else lddx
        self.dx_col0 = self.col0 if dx_col0 is None else dx_col0
        self.loss, self.pred = Buf((R,)), Buf((R,), dtype=torch.int32)
        self.h, self.g1, self.g2, self.dx = Buf((R, H)), Buf((R, H)), Buf((R, S)), Buf((R, self.lddx))
        self.dw1, self.db1, self.dw2, self.db2, self.out = Buf((H, self.ldw1)), Buf((H,)), Buf((S, H)), Buf((S,)), Buf((4,))

    def inputs(self):
        return [p.buf for p in (self.x, self.w1, self.b1, self.w2, self.b2, self.coef)] + [self.labels]

    def outputs(self):
        return [self.loss, self.pred, self.h, self.g1, self.g2, self.dx, self.dw1, self.db1, self.dw2, self.db2, self.out]

    def rows(self, rc=0, **kw):
        R, D, H, S = self.dims
        a = dict(x=self.x.buf.at(4 + self.col0), ldx=self.ldx, labels=self.labels.ptr, w1=self.w1.ptr, ldw1=self.ldw1,
                 b1=self.b1.ptr, w2=self.w2.ptr, b2=self.b2.ptr, coef=self.coef.ptr, inv_rows=self.inv_rows, R=R, D=D, H=H,
                 S=S, loss=self.loss.ptr, pred=self.pred.ptr, h=self.h.ptr, g2=self.g2.ptr, g1=self.g1.ptr, dx=self.dx.ptr,
                 lddx=self.lddx, dx_col0=self.dx_col0)
        a.update(kw)
        got = L().dvae_adv_rows(a["x"], a["ldx"], a["labels"], a["w1"], a["ldw1"], a["b1"], a["w2"], a["b2"], a["coef"],
                                a["inv_rows"], a["R"], a["D"], a["H"], a["S"], a["loss"], a["pred"], a["h"], a["g2"], a["g1"],
                                a["dx"], a["lddx"], a["dx_col0"], st())
        ok(got, "dvae_adv_rows") if rc == 0 else self.refused(got, rc)
        guards(*self.inputs(), *self.outputs())

    def params(self, rc=0, **kw):
        R, D, H, S = self.dims
        a = dict(x=self.x.buf.at(4 + self.col0), ldx=self.ldx, labels=self.labels.ptr, h=self.h.ptr, g2=self.g2.ptr,
                 g1=self.g1.ptr, loss=self.loss.ptr, pred=self.pred.ptr, inv_rows=self.inv_rows, R=R, D=D, H=H, S=S,
                 dw1=self.dw1.ptr, ldw1=self.ldw1, db1=self.db1.ptr, dw2=self.dw2.ptr, db2=self.db2.ptr, out=self.out.ptr)
        a.update(kw)
        got = L().dvae_adv_params(a["x"], a["ldx"], a["labels"], a["h"], a["g2"], a["g1"], a["loss"], a["pred"], a["inv_rows"],
                                  a["R"], a["D"], a["H"], a["S"], a["dw1"], a["ldw1"], a["db1"], a["dw2"], a["db2"], a["out"],
                                  st())
        ok(got, "dvae_adv_params") if rc == 0 else self.refused(got, rc)
        guards(*self.inputs(), *self.outputs())

    @staticmethod
    def refused(got, rc):
        assert got == rc, got

    def bits(self):
        return {k: getattr(self, k).bits() for k in ("loss", "pred", "h", "g1", "g2", "dx", "dw1", "db1", "dw2", "db2", "out")}


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", list(A.CASES))
def test_both_launches_against_float64(cases, name):
    c = cases[name]
    R, D, H, S = c["R"], c["D"], c["H"], c["S"]
    res, par, bnd = c["res"], c["par"], c["bnd"]
    n = Net(c)
    n.rows()
    n.params()
    got = dict(h=n.h.np(), loss=n.loss.np(), g2=n.g2.np(), g1=n.g1.np(), dx=n.dx.np(), dw1=n.dw1.np(), db1=n.db1.np(),
               dw2=n.dw2.np(), db2=n.db2.np(), out=n.out.np())
    for k in ROW_KEYS:
        note((name, k), got[k], res[k], bnd[k], k)
    lo, hi = n.col0, n.col0 + D
    note((name, "dx"), got["dx"][:, lo:hi], res["dx"], bnd["dx"], "dx")
    note((name, "dw1"), got["dw1"][:, :D], par["dw1"], bnd["dw1"], "dw1")
    for k in ("db1", "dw2", "db2"):
        note((name, k), got[k], par[k], bnd[k], k)
    note((name, "out"), got["out"][[0, 3]], par["out"][[0, 3]], bnd["out"][[0, 3]], "out")
    # exact: the arg-max, the counts, every zero the contract names
    assert np.array_equal(n.pred.np(), res["pred"])
    assert got["out"][1] == par["out"][1] and got["out"][2] == par["out"][2]
    dxb = n.dx.bits()
    assert not dxb[:, :lo].any() and not dxb[:, hi:].any(), "the columns of dx beside x's are +0.0"
    assert not n.dw1.bits()[:, D:].any(), "padding columns of dw1 are +0.0"
    for r in np.nonzero(~res["counted"])[0]:
        assert not n.loss.bits()[r] and not n.g2.bits()[r].any() and not n.g1.bits()[r].any() and not dxb[r].any(), \
            f"ignored row {r} is +0.0"
    assert (~(res["h"] > 0) == (n.h.bits() == 0)).all() and not n.g1.bits()[~(res["h"] > 0)].any()
    # a second pair of launches gives the same bits; so does evaluation (no gradients) for what it writes
    first = n.bits()
    n.new_outputs()
    n.rows()
    n.params()
    second = n.bits()
    for k in first:
        assert np.array_equal(first[k], second[k]), f"{k}: two launches"
    n.dw1, n.db1, n.dw2, n.db2, n.out = Buf((H, n.ldw1)), Buf((H,)), Buf((S, H)), Buf((S,)), Buf((4,))
    n.params(dw1=None, db1=None, dw2=None, db2=None)
    assert np.array_equal(n.out.bits(), first["out"])
    for k in GRAD_KEYS:
        untouched(getattr(n, k).bits(), f"{k} of an evaluation")


def test_a_row_does_not_depend_on_the_other_rows(cases):
    """row 7 of the step's case alone (R = 1, the same inv_rows) and among 128"""
    c = cases["step"]
    n = Net(c)
    n.rows()
    one = dict(c, R=1, x=c["x"][7:8], labels=c["labels"][7:8])
    m = Net(one)
    m.rows()
    for k in ("loss", "pred", "h", "g1", "g2", "dx"):
        assert np.array_equal(getattr(m, k).bits()[0], getattr(n, k).bits()[7]), k


def test_dense_dx(cases):
    """lddx = D, dx_col0 = 0 on a table whose x starts at column 2: the dense form of the contract"""
    c = cases["small"]
    n = Net(c)
    n.rows()
    ref = n.dx.bits()[:, n.col0:n.col0 + c["D"]]
    n.new_outputs(lddx=c["D"], dx_col0=0)
    n.rows()
    assert np.array_equal(n.dx.bits(), ref)


# ------------------------------------------------------------------------------------------- lambda = 0 and a NaN
@pytest.mark.parametrize("name", ["odd", "step"])
def test_lambda_zero_writes_plus_zero_whatever_the_row_holds(cases, name):
    c = cases[name]
    x = c["x"].copy()
    x[2, 0] = np.nan
    x[4 % c["R"], c["D"] - 1] = np.inf
    n = Net(c, lam=0.0, x=x)
    n.rows()
    n.params()
    # (relu drops the NaN row's pre-activations; the inf row's logits are inf - inf)
    assert np.isnan(n.g2.np()[4 % c["R"]]).any() and np.isnan(n.dw2.np()).any(), "the NaN is in the adversary"
    assert not n.dx.bits().any(), "dx is +0.0 in every bit"
    # -0.0 is zero too: the rule is on the device VALUE
    m = Net(c, lam=-0.0, x=x)
    m.rows()
    assert not m.dx.bits().any()
    # the clean rows are what they are under any lambda
    k = Net(c)
    k.rows()
    clean = [r for r in range(c["R"]) if r not in (2, 4 % c["R"])]
    for key in ("loss", "h", "g2", "g1"):
        assert np.array_equal(getattr(n, key).bits()[clean], getattr(k, key).bits()[clean]), key


# ------------------------------------------------------------------------------------------------------ EINVAL
def test_einval_writes_nothing(cases):
    c = cases["small"]
    R, D, H, S = c["R"], c["D"], c["H"], c["S"]
    n = Net(c)
    bad_rows = [dict(R=0), dict(D=0), dict(D=65), dict(H=0), dict(H=32), dict(H=96), dict(H=1088), dict(S=0), dict(S=1025),
                dict(ldx=D - 1), dict(ldw1=D - 1), dict(ldw1=D + 1), dict(ldw1=68), dict(dx_col0=-1), dict(lddx=n.dx_col0 + D - 1),
                dict(w1=n.w1.ptr + 4), dict(w2=n.w2.ptr + 8)]
    bad_rows += [{k: None} for k in ("x", "labels", "w1", "b1", "w2", "b2", "coef", "loss", "pred", "h", "g2", "g1", "dx")]
    for kw in bad_rows:
        n.rows(rc=EINVAL, **kw)
    bad_params = [dict(R=0), dict(D=0), dict(D=65), dict(H=32), dict(H=1088), dict(S=0), dict(S=1025), dict(ldx=D - 1),
                  dict(ldw1=D + 1), dict(dw1=None), dict(db2=None), dict(dw1=None, db1=None, dw2=None)]
    bad_params += [{k: None} for k in ("x", "labels", "h", "g2", "g1", "loss", "pred", "out")]
    for kw in bad_params:
        n.params(rc=EINVAL, **kw)
    for b in n.outputs():
        untouched(b.bits(), "an output of a refused call")
