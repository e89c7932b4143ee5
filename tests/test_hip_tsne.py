"""The latent-map kernels of csrc/tsne.hip (dvae_tsne_nn, dvae_tsne_affinities, dvae_tsne_forces, dvae_tsne_update; DESIGN.md
section 4.17) on the MI355X through the C ABI, against the float64 restatement of tests/tsne_ref.py.

Every figure is held to the bound derived in tsne_ref (from 2^-24 and the operation counts, not from what the kernels give)
against float64 on the rounded inputs; the nearest neighbours and the gains are compared exactly; what the contract calls
bit-exact is compared bit for bit: two launches, a row alone against the same row among 129 others.  Every buffer a launch
may write is a guarded one of tests/kernel_harness.py, pre-filled with 0xFF; inputs carry NaN wherever the entry point
must not read.  The worst error / bound per family is printed at the module's end.

Worst error / bound on the MI355X over the 56 shapes: d2min 0.700, lnz 0.254, entropy 0.173, the float64 entropy at the
device's beta against ln perplexity 0.904, A 0.354, R 0.116, Z 0.202, the KL sums 0.336, the KL from them 0.031, upd 0.927,
y 0.933, the update's float64 KL 0.002.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, F32, F64, guards, L, ok, Pad, st, untouched, Worst
import dvae_amd  # noqa: E402,F401
import tsne_ref as R  # noqa: E402
from ref_common import EPS32  # noqa: E402

WORST = Worst("test_hip_tsne.py (rows: D, ld)")
note = WORST.note
CASES = [(N, D, ld) for D, ld in R.SHAPES for N in R.NS]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def i32buf(a):
    return Buf(data=np.ascontiguousarray(a, np.int32))


class Dev:
    """a kernel_case on the device: x [N, ld] with NaN around it and in the columns D .. ld - 1, the groups"""

    def __init__(self, c, x=None):
        self.N, self.D, self.ld = c["N"], c["D"], c["ld"]
        full = c["full"]
        if x is not None:
            full = np.full((len(x), self.ld), np.nan, F32)
            full[:, :self.D] = x
        self.x = Pad(full)
        self.group = i32buf(c["group"])

    def nn(self, group=None, row0=0, nrows=None, rc=0, **kw):
        d2min, arg = Buf((self.N,)), Buf((self.N,), dtype=torch.int32)
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, D=self.D, group=group, row0=row0,
                 nrows=self.N if nrows is None else nrows, d2min=d2min.ptr, arg=arg.ptr)
        a.update(kw)
        got = L().dvae_tsne_nn(a["x"], a["ld"], a["N"], a["D"], a["group"], a["row0"], a["nrows"], a["d2min"], a["arg"], st())
        assert got == rc, (got, L().dvae_last_hip_error())
        guards(d2min, arg, self.x.buf, self.group)
        return d2min, arg

    def affinities(self, dm, perplexity, max_steps=R.MAX_STEPS, row0=0, nrows=None, rc=0, **kw):
        outs = [Buf((self.N,)) for _ in range(3)] + [Buf((self.N,), dtype=torch.int32)]
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, D=self.D, d2min=dm.ptr, perplexity=perplexity, max_steps=max_steps,
                 row0=row0, nrows=self.N if nrows is None else nrows, beta=outs[0].ptr, lnz=outs[1].ptr,
                 entropy=outs[2].ptr, steps=outs[3].ptr)
        a.update(kw)
        got = L().dvae_tsne_affinities(a["x"], a["ld"], a["N"], a["D"], a["d2min"], a["perplexity"], a["max_steps"],
                                       a["row0"], a["nrows"], a["beta"], a["lnz"], a["entropy"], a["steps"], st())
        assert got == rc, (got, L().dvae_last_hip_error())
        guards(*outs, self.x.buf)
        return outs

    def forces(self, t, yp, want_kl=1, row0=0, nrows=None, rc=0, **kw):
        rows = Buf((self.N, 8))
        a = dict(x=self.x.ptr, ld=self.ld, N=self.N, D=self.D, beta=t["beta"].ptr, d2min=t["d2min"].ptr, lnz=t["lnz"].ptr,
                 y=yp.ptr, want_kl=want_kl, row0=row0, nrows=self.N if nrows is None else nrows, rows=rows.ptr)
        a.update(kw)
        got = L().dvae_tsne_forces(a["x"], a["ld"], a["N"], a["D"], a["beta"], a["d2min"], a["lnz"], a["y"], a["want_kl"],
                                   a["row0"], a["nrows"], a["rows"], st())
        assert got == rc, (got, L().dvae_last_hip_error())
        guards(rows, self.x.buf, yp.buf, *(v.buf for v in t.values()))
        return rows


def tables(c):
    return {k: Pad(v) for k, v in R.forces_inputs(c).items()}


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("N,D,ld", CASES)
def test_nearest_against_float64(N, D, ld):
    c = R.kernel_case(N, D, ld)
    dev = Dev(c)
    key = f"{D},{ld}"
    for grp, gp in ((None, None), (c["group"], dev.group.ptr)):
        best, arg = R.nearest(c["d2"], grp)
        d2min, a = dev.nn(gp)
        assert np.array_equal(a.np(), arg), "the nearest admissible neighbour, ties to the lowest index"
        has = arg >= 0
        note((key, "nn"), d2min.np()[has], best[has], R.dist_bound(best[has], D), f"N={N} d2min")
        assert np.all(np.isposinf(d2min.np()[~has]))
        d2, a2 = dev.nn(gp)
        assert np.array_equal(d2.bits(), d2min.bits()) and np.array_equal(a2.bits(), a.bits()), "a second launch"
    assert a.np()[4] == 2 and dev.nn()[1].np()[2] == 3 and dev.nn()[1].np()[3] == 2      # the planted ties
    d2min, a = dev.nn(i32buf(np.zeros(N)).ptr)
    assert np.all(a.np() == -1) and np.all(np.isposinf(d2min.np())), "one group that covers every row"


@pytest.mark.parametrize("N,D,ld", CASES)
def test_affinities_against_float64(N, D, ld):
    c = R.kernel_case(N, D, ld)
    dev = Dev(c)
    key = f"{D},{ld}"
    perp = c["perplexity"]
    d2min, _ = dev.nn()
    beta, lnz, ent, steps = dev.affinities(d2min, perp)
    b64, dm64 = beta.np().astype(F64), d2min.np().astype(F64)
    assert np.all(steps.np() >= 1) and np.all(steps.np() <= R.MAX_STEPS), "every row converges inside the 64 evaluations"
    assert np.all(np.isfinite(b64)) and np.all(b64 > 0) and np.all(lnz.np() >= 0)
    l64, h64 = R.entropy_at(c["d2"], dm64, b64)
    bl, bh = R.affinities_bound(c["d2"], D, dm64, b64)
    note((key, "lnz"), lnz.np(), l64, bl, f"N={N} lnz")
    note((key, "entropy"), ent.np(), h64, bh, f"N={N} entropy")
    target = math.log(perp)
    tol = R.ENTROPY_TOL * (1.0 + 2.0 * EPS32) + bh + 2.0 * EPS32 * (np.abs(h64) + target)
    note((key, "perplexity"), h64, np.full(N, target), tol, f"N={N}: the float64 entropy at the device's beta")
    again = dev.affinities(d2min, perp)
    for o1, o2 in zip((beta, lnz, ent, steps), again):
        assert np.array_equal(o1.bits(), o2.bits()), "a second launch"


def test_more_ties_than_the_perplexity_come_back_unconverged():
    c = R.kernel_case(63, 4, 4)
    x = c["x"].copy()
    x[10:17] = x[10]
    dev = Dev(c, x)
    d2min, _ = dev.nn()
    beta, lnz, ent, steps = dev.affinities(d2min, 5.0)
    s = steps.np()
    assert np.all(s[10:17] == -1) and np.all(np.delete(s, np.s_[10:17]) >= 1)
    for b in (beta, lnz, ent):
        assert np.all(np.isfinite(b.np()))
    assert np.all(d2min.np()[10:17] == 0) and np.all(ent.np()[10:17] > math.log(6.0) - 1e-4)
    assert np.all(beta.np()[10:17] == 2.0 ** 63)      # doubled 63 times from 1: the last iterate, not one step further


@pytest.mark.parametrize("N,D,ld", CASES)
def test_forces_against_float64(N, D, ld):
    c = R.kernel_case(N, D, ld)
    dev = Dev(c)
    key = f"{D},{ld}"
    t, y = tables(c), Pad(c["y"])
    t64 = {k: v.astype(F64) for k, v in R.forces_inputs(c).items()}
    rows = dev.forces(t, y, 1)
    ref = R.row_sums(R.dense_P(c["d2"], t64["beta"], t64["d2min"], t64["lnz"]), c["y"])
    fb = R.forces_bound(c["d2"], D, t64["beta"], t64["d2min"], t64["lnz"], c["y"])
    got = rows.np()
    for name, sl in (("A", slice(0, 2)), ("R", slice(2, 4)), ("Z", slice(4, 5)), ("kl sums", slice(5, 8))):
        note((key, name), got[:, sl], ref[:, sl], fb[:, sl], f"N={N} {name}")
    kb = fb[:, 5].sum() + fb[:, 6].sum() + abs(math.log(ref[:, 4].sum())) * fb[:, 7].sum() \
        + fb[:, 4].sum() / (ref[:, 4].sum() - fb[:, 4].sum()) * (ref[:, 7].sum() + fb[:, 7].sum())
    note((key, "KL"), [R.kl_of(got)], [R.kl_of(ref)], [kb], f"N={N} KL")
    plain = dev.forces(t, y, 0).np()
    assert np.array_equal(plain[:, :5].view(np.uint32), got[:, :5].view(np.uint32)), "the five sums do not depend on want_kl"
    assert np.all(plain[:, 5:].view(np.uint32) == 0), "want_kl = 0 leaves the KL columns +0"
    assert np.array_equal(dev.forces(t, y, 1).bits(), rows.bits()), "a second launch"


@pytest.mark.parametrize("N,D,ld", CASES)
def test_update_against_float64(N, D, ld):
    c = R.kernel_case(N, D, ld)
    u = R.update_case(c)
    key = f"{D},{ld}"
    rows = Pad(u["rows"])
    y, upd, gains, kl = Buf(data=c["y"]), Buf(data=u["upd"]), Buf(data=u["gains"]), Buf((1,), dtype=torch.float64)
    ok(L().dvae_tsne_update(rows.ptr, N, y.ptr, upd.ptr, gains.ptr, u["lr"], u["momentum"], u["ex"], kl.ptr, st()),
       "dvae_tsne_update")
    guards(y, upd, gains, kl, rows.buf)
    ref, b = u["ref"], u["bound"]
    assert np.array_equal(gains.np().view(np.uint32), ref["gains"].view(np.uint32)), "the gains are exact"
    note((key, "upd"), upd.np(), ref["upd"], b["upd"], f"N={N} upd")
    note((key, "y"), y.np(), ref["y"], b["y"], f"N={N} y")
    note((key, "kl"), kl.np(), [ref["kl"]], [b["kl"]], f"N={N} kl")
    # without a KL slot the same update, and the same bits from a second launch
    y2, upd2, gains2 = Buf(data=c["y"]), Buf(data=u["upd"]), Buf(data=u["gains"])
    ok(L().dvae_tsne_update(rows.ptr, N, y2.ptr, upd2.ptr, gains2.ptr, u["lr"], u["momentum"], u["ex"], None, st()))
    guards(y2, upd2, gains2)
    for o1, o2 in ((y, y2), (upd, upd2), (gains, gains2)):
        assert np.array_equal(o1.bits(), o2.bits())


# ----------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("D,ld", [(5, 7), (32, 33)])
def test_a_row_alone_and_among_others(D, ld):
    N = 257
    c = R.kernel_case(N, D, ld)
    dev = Dev(c)
    t, y = tables(c), Pad(c["y"])
    all_d, all_a = dev.nn(dev.group.ptr)
    plain_d, _ = dev.nn()
    all_aff = dev.affinities(plain_d, 5.0)
    all_rows = dev.forces(t, y, 1)
    for row0, nrows in ((0, 130), (0, 1), (1, 1), (64, 1), (129, 1), (200, 57)):
        sl = slice(row0, row0 + nrows)
        d, a = dev.nn(dev.group.ptr, row0, nrows)
        aff = dev.affinities(plain_d, 5.0, row0=row0, nrows=nrows)
        rows = dev.forces(t, y, 1, row0, nrows)
        for part, whole, what in [(d, all_d, "d2min"), (a, all_a, "arg"), (rows, all_rows, "rows")] + \
                                 [(p, w, "affinities") for p, w in zip(aff, all_aff)]:
            pb, wb = part.bits(), whole.bits()
            assert np.array_equal(pb[sl], wb[sl]), f"{what}: rows {row0}..{row0 + nrows} alone and among {N}"
            untouched(pb[:row0], f"{what}: rows in front")
            untouched(pb[row0 + nrows:], f"{what}: rows behind")


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    c = R.kernel_case(65, 5, 7)
    dev = Dev(c)
    t, y = tables(c), Pad(c["y"])
    big = Pad(np.zeros((65, 80), F32))
    for kw in (dict(x=None), dict(d2min=None), dict(arg=None), dict(N=0), dict(D=0), dict(D=65, ld=80, x=big.ptr), dict(ld=4),
               dict(row0=-1), dict(nrows=-1), dict(row0=60, nrows=6), dict(N=2 ** 31)):
        outs = dev.nn(rc=EINVAL, **kw)
        assert all(o.poisoned().all() for o in outs), kw
    assert all(o.poisoned().all() for o in dev.nn(nrows=0))      # a no-op
    d2min, _ = dev.nn()
    for kw in (dict(x=None), dict(d2min=None), dict(beta=None), dict(lnz=None), dict(entropy=None), dict(steps=None),
               dict(D=0), dict(D=65, ld=80, x=big.ptr), dict(ld=4), dict(row0=-1), dict(row0=1, nrows=65),
               dict(perplexity=0.5), dict(perplexity=65.0), dict(perplexity=float("nan")), dict(max_steps=0), dict(N=1, nrows=1)):
        kw = dict(kw)
        outs = dev.affinities(d2min, kw.pop("perplexity", 5.0), rc=EINVAL, **kw)
        assert all(o.poisoned().all() for o in outs), kw
    assert all(o.poisoned().all() for o in dev.affinities(d2min, 5.0, nrows=0))
    for kw in (dict(x=None), dict(beta=None), dict(d2min=None), dict(lnz=None), dict(y=None), dict(rows=None), dict(D=0),
               dict(D=65, ld=80, x=big.ptr), dict(ld=4), dict(want_kl=2), dict(want_kl=-1), dict(row0=-1), dict(nrows=66),
               dict(N=0, nrows=0)):
        assert dev.forces(t, y, rc=EINVAL, **kw).poisoned().all(), kw
    assert dev.forces(t, y, nrows=0).poisoned().all()
    u = R.update_case(c)
    rows = Pad(u["rows"])
    for kw in (dict(rows=None), dict(y=None), dict(upd=None), dict(gains=None), dict(N=0), dict(N=-3), dict(lr=0.0),
               dict(lr=float("nan")), dict(momentum=-0.1), dict(ex=0.0), dict(kl=4)):
        yb, ub, gb, kl = Buf((65, 2)), Buf((65, 2)), Buf((65, 2)), Buf((2,), dtype=torch.float64)
        a = dict(rows=rows.ptr, N=65, y=yb.ptr, upd=ub.ptr, gains=gb.ptr, lr=200.0, momentum=0.5, ex=12.0, kl=0)
        a.update(kw)
        klp = None if a["kl"] is None else kl.ptr + a["kl"]
        rc = L().dvae_tsne_update(a["rows"], a["N"], a["y"], a["upd"], a["gains"], a["lr"], a["momentum"], a["ex"], klp, st())
        assert rc == EINVAL, kw
        guards(yb, ub, gb, kl)
        assert all(b.poisoned().all() for b in (yb, ub, gb, kl)), kw
