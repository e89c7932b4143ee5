"""The batch-norm kernels on the MI355X (csrc/bn.hip: dvae_bn_stats_fwd, dvae_bn_stats_finalize, dvae_bn_apply_fwd,
dvae_bn_bwd, dvae_bn_bwd_from_y) against the float64 reference of tests/bn_ref.py, element by element and channel by channel.

Every comparison is ONE launch judged from its own inputs: what the launch reads is downloaded — the device's own fp32 mean
and rstd, its Z for dvae_bn_bwd, its s1 / s2 for dY — `bn_ref` runs on that in float64, and the result is compared with
what the launch left.  The bounds are the rounding bounds derived in tests/bn_ref.py (eps32 = 2^-24), per element or per
channel, never a fraction of a tensor's maximum.  bf16 stores have no bound: they must be bit-equal to the
round-to-nearest-even bf16 of the fp32 output of the same launch made with fp32 storage.

Every buffer a launch may write, the workspace of dvae_bn_ws_bytes included, is a guarded one of tests/kernel_harness.py.
bn.hip does not read the compute mode, so nothing is parametrised over it.  The worst error / bound per quantity over the
module is printed at its end.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, guards, L, P, st, sync, Worst      # first: it puts the repository root on sys.path
import bn_ref as B  # noqa: E402

EPSF, MOMF = np.float32(1e-5), np.float32(0.1)
ACTS = {"none": B.ACT_NONE, "relu": B.ACT_RELU, "tanh": B.ACT_TANH}
CASE_IDS = ["x".join(map(str, c)) for c in B.CASES]
BIG = B.CASES[-1]
WORST = Worst("test_hip_bn.py", ratio_fn=B.worst_ratio)      # quantity -> worst error / bound over this module
note = WORST.note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def workspace(R, C, G):
    """dvae_bn_ws_bytes of 0xFF inside guards.  The partials and s12 end 64 bytes before the size the library asks for: that
    tail must keep its poison through every launch (`guards`), so an overrun of s12 shows as the guards' would."""
    ws = Buf((L().dvae_bn_ws_bytes(R, C, G),), torch.uint8)
    ws.slack_from = B.n_chunks(R) * G * C * 2 * 8 + G * C * 2 * 4
    assert 0 < ws.nbytes - ws.slack_from <= 64
    return ws


def s12_of(ws, R, C, G):
    """The fp32 (s1, s2) [G, C, 2] the backward finalize left behind the partials."""
    sync()
    off = B.n_chunks(R) * G * C * 2 * 8
    return ws.t[off:off + G * C * 8].view(torch.float32).view(G, C, 2).cpu().numpy().copy()


def rne_bf16_bits(buf):
    """Bits of the round-to-nearest-even bf16 of an fp32 buffer."""
    sync()
    return buf.t.to(torch.bfloat16).view(torch.int16).cpu().numpy()


class Ctx:
    """One case's inputs on the host and on the device, the device's own statistics, and (lazily) its own Z per activation."""

    def __init__(self, case):
        self.case = case
        R, N, G, C = case
        self.d = B.make_inputs(R, N, G, C, B.SEEDS[case])
        self.y, self.dz, self.res = (Buf((R, C), data=self.d[k]) for k in ("y", "dz", "res"))
        self.gamma, self.beta = Buf((C,), data=self.d["gamma"]), Buf((C,), data=self.d["beta"])
        self.mean, self.rstd = Buf((G, C)), Buf((G, C))
        ws = workspace(R, C, G)
        assert L().dvae_bn_stats_fwd(self.y.ptr, self.mean.ptr, self.rstd.ptr, None, None, None, ws.ptr, R, N, C, G,
                                     float(EPSF), float(MOMF), st()) == 0
        guards(self.mean, self.rstd, ws)
        self.mean_np, self.rstd_np = self.mean.np(), self.rstd.np()
        assert np.isfinite(self.mean_np).all() and np.isfinite(self.rstd_np).all()
        self.zs = {}

    def z(self, act, b16=False):
        if (act, b16) not in self.zs:
            R, N, G, C = self.case
            z = Buf((R, C), torch.bfloat16 if b16 else torch.float32)
            apply_fwd(self, z, act, None)
            self.zs[(act, b16)] = z
        return self.zs[(act, b16)]


@functools.lru_cache(maxsize=None)
def ctx(case):
    return Ctx(case)


def apply_fwd(c, z, act, res):
    R, N, G, C = c.case
    rc = L().dvae_bn_apply_fwd(c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, c.beta.ptr, P(res), z.ptr, R, N, C, G, act,
                               int(z.dtype == torch.bfloat16), st())
    assert rc == 0
    guards(z)


def launch_bwd(c, act, from_y, z=None, dy=None, dgamma=None, dbeta=None, ws=None, dz=None, dy_ptr=None):
    """dvae_bn_bwd (from_y False: reads `z`) or dvae_bn_bwd_from_y.  Returns the return code."""
    R, N, G, C = c.case
    dz = c.dz if dz is None else dz
    dtypes = (2 if dy is not None and dy.dtype == torch.bfloat16 else 0) | (1 if z is not None and z.dtype == torch.bfloat16 else 0)
    dyp = dy.ptr if dy_ptr is None else dy_ptr
    if from_y:
        rc = L().dvae_bn_bwd_from_y(dz.ptr, c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, c.beta.ptr, dyp, P(dgamma), P(dbeta),
                                    P(ws), R, N, C, G, act, dtypes, st())
    else:
        rc = L().dvae_bn_bwd(dz.ptr, c.y.ptr, P(z), c.mean.ptr, c.rstd.ptr, c.gamma.ptr, dyp, P(dgamma), P(dbeta), P(ws),
                             R, N, C, G, act, dtypes, st())
    sync()
    return rc


def judged_bwd(c, act, from_y, z, what):
    """One fp32-dY launch onto non-zero dgamma / dbeta, judged from its inputs.  Returns (dy, dgamma, dbeta) buffers."""
    R, N, G, C = c.case
    d = c.d
    dy, dg, db, ws = Buf((R, C)), Buf((C,), data=d["dgamma0"]), Buf((C,), data=d["dbeta0"]), workspace(R, C, G)
    assert launch_bwd(c, act, from_y, z=z, dy=dy, dgamma=dg, dbeta=db, ws=ws) == 0
    guards(dy, dg, db, ws)
    s12 = s12_of(ws, R, C, G)
    zin = None if from_y else z.np()
    assert np.isfinite(s12).all() and (zin is None or np.isfinite(zin).all()), f"{what}: the launch's own Z or s12 is not finite"
    bb = B.bwd_bounds(d["dz"], d["y"], zin, c.mean_np, c.rstd_np, d["gamma"], d["beta"], N, G, act, d["dgamma0"], d["dbeta0"], s12=s12)
    amb = None
    if from_y and act == B.ACT_RELU:
        amb = B.ambiguous_pairs(d["y"], c.mean_np, c.rstd_np, d["gamma"], d["beta"], N, G)
        assert amb.mean() <= 0.005, f"{what}: {int(amb.sum())} of {amb.size} (group, channel) pairs hold a pre-activation within the forward bound of 0"
    amb_c = None if amb is None else amb.any(0)
    amb_r = None if amb is None else amb[B.groups(R, N, G)]
    note("s1", s12[..., 0], bb["s1"], bb["tol_s1"], what, amb)
    note("s2", s12[..., 1], bb["s2"], bb["tol_s2"], what, amb)
    note("dgamma", dg.np(), bb["dgamma"], bb["tol_dgamma"], what, amb_c)
    note("dbeta", db.np(), bb["dbeta"], bb["tol_dbeta"], what, amb_c)
    note("dy", dy.np(), bb["dy"], bb["tol_dy"], what, amb_r)
    return dy, dg, db


# ------------------------------------------------------------------ the entry points at every shape
@pytest.mark.parametrize("case", B.CASES, ids=CASE_IDS)
def test_stats_fwd(case):
    R, N, G, C = case
    c = ctx(case)
    d = c.d
    mean, rstd, rm, rv = Buf((G, C)), Buf((G, C)), Buf((C,), data=d["rm0"]), Buf((C,), data=d["rv0"])
    nbt, ws = Buf((1,), torch.int64, data=np.array([7], np.int64)), workspace(R, C, G)
    assert L().dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, ws.ptr, R, N, C, G, float(EPSF),
                                 float(MOMF), st()) == 0
    guards(mean, rstd, rm, rv, nbt, ws)
    sb = B.stats_bounds(d["y"], N, G, EPSF, d["rm0"], d["rv0"], MOMF)
    what = f"stats_fwd {case}"
    note("mean", mean.np(), sb["mean"], sb["tol_mean"], what)
    note("rstd", rstd.np(), sb["rstd"], sb["tol_rstd"], what)
    note("running_mean", rm.np(), sb["rm"], sb["tol_rm"], what)
    note("running_var", rv.np(), sb["rv"], sb["tol_rv"], what)
    assert int(nbt.np()[0]) == 7 + G
    assert np.array_equal(mean.bits(), c.mean.bits()) and np.array_equal(rstd.bits(), c.rstd.bits())     # null running_*: same statistics
    if B.count(R, N, G) == 1:                                   # one value per channel and group: the kernel's rule
        assert np.array_equal(mean.np(), d["y"].reshape(G, C)) and (rstd.np() == np.float32(float(EPSF) ** -0.5)).all()


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", B.CASES, ids=CASE_IDS)
def test_apply_fwd(case, act):
    R, N, G, C = case
    c, a = ctx(case), ACTS[act]
    z = c.z(a)
    ab = B.apply_bounds(c.d["y"], c.mean_np, c.rstd_np, c.d["gamma"], c.d["beta"], None, N, G, a)
    note("z_" + act, z.np(), ab["z"], ab["tol_z"], f"apply_fwd {case} {act}")
    assert np.array_equal(c.z(a, b16=True).bits(), rne_bf16_bits(z)), "bf16 Z is not the RNE of the fp32 Z"


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", B.CASES, ids=CASE_IDS)
def test_bwd(case, act):
    """dvae_bn_bwd with the device's own Z, fp32 and bf16, dY fp32 and bf16 (dtypes 0, 2, 1, 3)."""
    R, N, G, C = case
    c, a = ctx(case), ACTS[act]
    for b16 in (False, True):
        z = c.z(a, b16)
        dy, dg, db = judged_bwd(c, a, False, z, f"bwd {case} {act} Z {'bf16' if b16 else 'fp32'}")
        dy16, dg2, db2, ws = Buf((R, C), torch.bfloat16), Buf((C,), data=c.d["dgamma0"]), Buf((C,), data=c.d["dbeta0"]), workspace(R, C, G)
        assert launch_bwd(c, a, False, z=z, dy=dy16, dgamma=dg2, dbeta=db2, ws=ws) == 0
        guards(dy16, dg2, db2, ws)
        assert np.array_equal(dy16.bits(), rne_bf16_bits(dy)), "bf16 dY is not the RNE of the fp32 dY"
        assert np.array_equal(dg2.bits(), dg.bits()) and np.array_equal(db2.bits(), db.bits())


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("case", B.CASES, ids=CASE_IDS)
def test_bwd_from_y(case, act):
    R, N, G, C = case
    c, a = ctx(case), ACTS[act]
    dy, dg, db = judged_bwd(c, a, True, None, f"bwd_from_y {case} {act}")
    dy16, dg2, db2, ws = Buf((R, C), torch.bfloat16), Buf((C,), data=c.d["dgamma0"]), Buf((C,), data=c.d["dbeta0"]), workspace(R, C, G)
    assert launch_bwd(c, a, True, dy=dy16, dgamma=dg2, dbeta=db2, ws=ws) == 0
    guards(dy16, dg2, db2, ws)
    assert np.array_equal(dy16.bits(), rne_bf16_bits(dy)), "bf16 dY is not the RNE of the fp32 dY"
    assert np.array_equal(dg2.bits(), dg.bits()) and np.array_equal(db2.bits(), db.bits())


@pytest.mark.parametrize("act", list(ACTS))
@pytest.mark.parametrize("case", [B.CASES[2], B.CASES[3]], ids=[CASE_IDS[2], CASE_IDS[3]])
def test_residual_is_added_after_the_activation(case, act):
    R, N, G, C = case
    c, a = ctx(case), ACTS[act]
    z, z16 = Buf((R, C)), Buf((R, C), torch.bfloat16)
    apply_fwd(c, z, a, c.res)
    apply_fwd(c, z16, a, c.res)
    ab = B.apply_bounds(c.d["y"], c.mean_np, c.rstd_np, c.d["gamma"], c.d["beta"], c.d["res"], N, G, a)
    note("z_" + act + "_residual", z.np(), ab["z"], ab["tol_z"], f"apply_fwd + residual {case} {act}")
    assert np.array_equal(z16.bits(), rne_bf16_bits(z))
    if a != B.ACT_NONE:                           # the data tells act(u) + r from act(u + r): they differ by far more than the bound
        _, wrong = B.apply(c.d["y"], c.mean_np, c.rstd_np, c.d["gamma"], c.d["beta"], None, N, G, B.ACT_NONE)
        wrong = B.act_apply(wrong + c.d["res"], a)
        assert (np.abs(wrong - ab["z"]) > 100 * ab["tol_z"]).mean() > 0.2


# ------------------------------------------------------------------ dvae_bn_stats_finalize alone, on partials the host wrote
CHUNKS = [1, 2, 63, 64, 65, 128, 192, 193, 194, 255, 256, 257, 320, 449, 1025]


@pytest.mark.parametrize("chunks", CHUNKS)
def test_finalize_alone_on_host_partials(chunks):
    """Every loop boundary of sum_partials: a dropped or doubled chunk moves the mean by parts in a thousand."""
    ragged = CHUNKS.index(chunks) % 2 == 1
    for C in (8, 80):
        for G in (1, 2):
            N = G
            R = 64 * chunks - (26 if ragged else 0)
            assert B.n_chunks(R) == chunks and R % N == 0
            rs = np.random.RandomState(1000 * chunks + 10 * C + G)
            gi = B.groups(R, N, G)
            y = rs.uniform(-3, 3, C) + 0.7 * gi[:, None] + rs.uniform(0.05, 2, C) * rs.standard_normal((R, C))
            part = np.zeros((chunks, G, C, 2))
            for k in range(G):
                yk = np.zeros((chunks * 64, C))
                yk[:R] = y * (gi == k)[:, None]
                yk = yk.reshape(chunks, 64, C)
                part[:, k, :, 0], part[:, k, :, 1] = yk.sum(1), (yk * yk).sum(1)
            ws = workspace(R, C, G)
            ws.t[:part.size * 8].copy_(torch.from_numpy(part.reshape(-1)).view(torch.uint8).to(ws.t.device))
            rm0, rv0 = rs.uniform(-1, 1, C).astype(np.float32), rs.uniform(0.5, 1.5, C).astype(np.float32)
            rm, rv, nbt = Buf((C,), data=rm0), Buf((C,), data=rv0), Buf((1,), torch.int64, data=np.array([3], np.int64))
            first = None
            for call in (1, 2):
                mean, rstd = Buf((G, C)), Buf((G, C))
                assert L().dvae_bn_stats_finalize(mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, ws.ptr, R, N, C, G, float(EPSF),
                                                  float(MOMF), st()) == 0
                guards(mean, rstd, rm, rv, nbt, ws)
                sb = B.stats_bounds(y, N, G, EPSF, rm0, rv0, MOMF, from_partials=True)
                what = f"finalize chunks={chunks} R={R} C={C} G={G} call {call}"
                note("mean", mean.np(), sb["mean"], sb["tol_mean"], what)
                note("rstd", rstd.np(), sb["rstd"], sb["tol_rstd"], what)
                note("running_mean", rm.np(), sb["rm"], sb["tol_rm"], what)
                note("running_var", rv.np(), sb["rv"], sb["tol_rv"], what)
                assert int(nbt.np()[0]) == 3 + call * G
                rm0, rv0 = rm.np(), rv.np()                      # the second call starts from what the first left
                if first is not None:
                    assert np.array_equal(first[0], mean.bits()) and np.array_equal(first[1], rstd.bits())
                first = (mean.bits(), rstd.bits())


# ------------------------------------------------------------------ parameters of the statistics
def test_momentum_eps_and_null_running_statistics():
    case = B.CASES[3]
    R, N, G, C = case
    c = ctx(case)
    d = c.d
    for eps in (1e-5, 1e-3):
        plain = None
        for mom in (0.1, 0.5, 1.0, 0.0):
            e, m = np.float32(eps), np.float32(mom)
            mean, rstd, rm, rv = Buf((G, C)), Buf((G, C)), Buf((C,), data=d["rm0"]), Buf((C,), data=d["rv0"])
            nbt, ws = Buf((1,), torch.int64, data=np.array([0], np.int64)), workspace(R, C, G)
            assert L().dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, ws.ptr, R, N, C, G, float(e), float(m), st()) == 0
            guards(mean, rstd, rm, rv, nbt, ws)
            sb = B.stats_bounds(d["y"], N, G, e, d["rm0"], d["rv0"], m)
            what = f"eps={eps} momentum={mom}"
            note("mean", mean.np(), sb["mean"], sb["tol_mean"], what)
            note("rstd", rstd.np(), sb["rstd"], sb["tol_rstd"], what)
            note("running_mean", rm.np(), sb["rm"], sb["tol_rm"], what)
            note("running_var", rv.np(), sb["rv"], sb["tol_rv"], what)
            assert int(nbt.np()[0]) == G
            if mom == 0.0:
                assert np.array_equal(rm.np(), d["rm0"]) and np.array_equal(rv.np(), d["rv0"])
            if plain is None:
                plain = (mean.bits(), rstd.bits(), rm.bits(), rv.bits())
        # null running_mean / running_var, then a null num_batches_tracked: everything else keeps its bits (momentum 0.1)
        m = np.float32(0.1)
        mean, rstd, nbt, ws = Buf((G, C)), Buf((G, C)), Buf((1,), torch.int64, data=np.array([0], np.int64)), workspace(R, C, G)
        assert L().dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, None, None, nbt.ptr, ws.ptr, R, N, C, G, float(e), float(m), st()) == 0
        guards(mean, rstd, nbt, ws)
        assert np.array_equal(mean.bits(), plain[0]) and np.array_equal(rstd.bits(), plain[1]) and int(nbt.np()[0]) == G
        mean, rstd, rm, rv, ws = Buf((G, C)), Buf((G, C)), Buf((C,), data=d["rm0"]), Buf((C,), data=d["rv0"]), workspace(R, C, G)
        assert L().dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, None, ws.ptr, R, N, C, G, float(e), float(m), st()) == 0
        guards(mean, rstd, rm, rv, ws)
        assert all(np.array_equal(a, b) for a, b in zip((mean.bits(), rstd.bits(), rm.bits(), rv.bits()), plain))


def test_one_pass_variance_under_cancellation():
    """R = 4096, standard deviation 1e-2 around 0, 1, 1e1 ... 1e5 and a constant channel at 1e4: mean and rstd inside the
    derived bound at each kappa = mean^2 / var (tests/bn_ref.py: the fp64 cancellation term stays below one fp32 rounding
    up to kappa = 1.2e7; the model reaches 1e6).  The table goes to DESIGN.md section 5."""
    R, C = 4096, 8
    y = B.cancellation_inputs(R)
    yb, mean, rstd, ws = Buf((R, C), data=y), Buf((1, C)), Buf((1, C)), workspace(R, C, 1)
    assert L().dvae_bn_stats_fwd(yb.ptr, mean.ptr, rstd.ptr, None, None, None, ws.ptr, R, 1, C, 1, float(EPSF), float(MOMF), st()) == 0
    guards(mean, rstd, ws)
    sb = B.stats_bounds(y, 1, 1, EPSF)
    m, r = mean.np()[0].astype(np.float64), rstd.np()[0].astype(np.float64)
    print("\nchannel | kappa | rstd error / eps32 rstd | bound / eps32 rstd | mean error / eps32 |mean|")
    for j in range(C):
        print(f"{j} | {sb['kappa'][0, j]:.3g} | {abs(r[j] - sb['rstd'][0, j]) / (B.EPS32 * sb['rstd'][0, j]):.3g} | "
              f"{sb['tol_rstd'][0, j] / (B.EPS32 * sb['rstd'][0, j]):.3g} | {abs(m[j] - sb['mean'][0, j]) / (B.EPS32 * max(abs(sb['mean'][0, j]), 1e-30)):.3g}")
    note("mean", m, sb["mean"][0], sb["tol_mean"][0], "cancellation")
    note("rstd_cancellation", r, sb["rstd"][0], sb["tol_rstd"][0], "cancellation")
    # what the model can produce (|mean| / std <= 1e3: channels 0..2 here) is held to fp32 rounding by that bound
    assert (sb["tol_rstd"][0, :3] < 1.1 * B.EPS32 * sb["rstd"][0, :3]).all()


# ------------------------------------------------------------------ exact-zero pre-activations
def test_exact_zero_preactivations():
    R, C, y, gamma, beta, dz = B.exact_zero_case()
    c = Ctx.__new__(Ctx)
    c.case, c.d = (R, 1, 1, C), {"y": y}
    c.y, c.dz, c.gamma, c.beta = Buf((R, C), data=y), Buf((R, C), data=dz), Buf((C,), data=gamma), Buf((C,), data=beta)
    mean, rstd = np.full((1, C), 0.5, np.float32), np.full((1, C), 2.0, np.float32)
    c.mean, c.rstd, c.zs = Buf((1, C), data=mean), Buf((1, C), data=rstd), {}
    u, _ = B.apply(y, mean, rstd, gamma, beta, None, 1, 1, B.ACT_NONE)
    assert (u == 0).sum() > R * C // 4 and (u > 0).sum() > R * C // 4 and (u < 0).sum() > R * C // 4
    for a in (B.ACT_NONE, B.ACT_RELU):
        z = c.z(a)
        zr = B.act_apply(u, a)
        assert np.array_equal(z.np().astype(np.float64), zr), "forward"
        if a == B.ACT_RELU:
            assert not z.bits()[u <= 0].any(), "ReLU of a pre-activation of -0 or below is +0"
        for from_y in (False, True):
            dy, dg, db, ws = Buf((R, C)), Buf((C,), data=np.zeros(C, np.float32)), Buf((C,), data=np.zeros(C, np.float32)), workspace(R, C, 1)
            assert launch_bwd(c, a, from_y, z=None if from_y else z, dy=dy, dgamma=dg, dbeta=db, ws=ws) == 0
            guards(dy, dg, db, ws)
            du, s1, s2, dgam, dbet, dyr = B.bwd(dz, y, None if from_y else zr, mean, rstd, gamma, beta, 1, 1, a)
            if a == B.ACT_RELU:                 # derivative 0 at u = +-0, 1 or 0 by sign next to it
                assert np.array_equal(du, np.where(u > 0, dz.astype(np.float64), 0.0))
            s12 = s12_of(ws, R, C, 1)
            what = f"act {a} from_y {from_y}"
            assert np.array_equal(s12[0, :, 0], s1[0].astype(np.float32)), what
            assert np.array_equal(s12[0, :, 1], s2[0].astype(np.float32)), what
            assert np.array_equal(db.np(), dbet.astype(np.float32)) and np.array_equal(dg.np(), dgam.astype(np.float32)), what
            assert np.array_equal(dy.np(), dyr.astype(np.float32)), what


# ------------------------------------------------------------------ contract lines
@pytest.mark.parametrize("from_y", [False, True], ids=["bwd", "bwd_from_y"])
def test_null_dgamma_dbeta_and_in_place(from_y):
    """dgamma / dbeta null: dY keeps its bits and the other one is still accumulated.  dY == dZ with an fp32 dY: the same
    dY, dgamma, dbeta bit for bit as out of place."""
    case = B.CASES[3]
    R, N, G, C = case
    c, a = ctx(case), B.ACT_RELU
    z = None if from_y else c.z(a)
    dy, dg, db = judged_bwd(c, a, from_y, z, f"reference launch from_y={from_y}")
    for null in ("both", "dgamma", "dbeta"):
        dy2, ws = Buf((R, C)), workspace(R, C, G)
        dg2 = None if null in ("both", "dgamma") else Buf((C,), data=c.d["dgamma0"])
        db2 = None if null in ("both", "dbeta") else Buf((C,), data=c.d["dbeta0"])
        assert launch_bwd(c, a, from_y, z=z, dy=dy2, dgamma=dg2, dbeta=db2, ws=ws) == 0
        guards(dy2, dg2, db2, ws)
        assert np.array_equal(dy2.bits(), dy.bits()), null
        assert dg2 is None or np.array_equal(dg2.bits(), dg.bits())
        assert db2 is None or np.array_equal(db2.bits(), db.bits())
    dzc, dg3, db3, ws = Buf((R, C), data=c.d["dz"]), Buf((C,), data=c.d["dgamma0"]), Buf((C,), data=c.d["dbeta0"]), workspace(R, C, G)
    assert launch_bwd(c, a, from_y, z=z, dy=dzc, dgamma=dg3, dbeta=db3, ws=ws, dz=dzc) == 0
    guards(dzc, dg3, db3, ws)
    assert np.array_equal(dzc.bits(), dy.bits()) and np.array_equal(dg3.bits(), dg.bits()) and np.array_equal(db3.bits(), db.bits())


@pytest.mark.parametrize("from_y", [False, True], ids=["bwd", "bwd_from_y"])
def test_in_place_bf16_dy_is_refused_and_nothing_is_written(from_y):
    """dY == dZ with dtypes bit 1: a bf16 quad would land on fp32 dZ another thread has yet to read (include/dvae_hip.h)."""
    case = B.CASES[2]
    R, N, G, C = case
    c = ctx(case)
    z = None if from_y else c.z(B.ACT_RELU)
    dzc, dg, db, ws = Buf((R, C), data=c.d["dz"]), Buf((C,), data=c.d["dgamma0"]), Buf((C,), data=c.d["dbeta0"]), workspace(R, C, G)
    before = (dzc.bits(), dg.bits(), db.bits())
    fake16 = Buf((1,), torch.bfloat16)                       # only its dtype is used: the pointer passed is dZ's
    assert launch_bwd(c, B.ACT_RELU, from_y, z=z, dy=fake16, dgamma=dg, dbeta=db, ws=ws, dz=dzc, dy_ptr=dzc.ptr) == EINVAL
    guards(dzc, dg, db, ws)
    assert all(np.array_equal(x, y) for x, y in zip(before, (dzc.bits(), dg.bits(), db.bits())))
    assert (ws.bits() == 0xFF).all()


def test_two_launches_are_bit_equal():
    case = BIG
    R, N, G, C = case
    c, d = ctx(case), ctx(case).d
    out = []
    for _ in range(2):
        o = []
        mean, rstd, rm, rv, ws = Buf((G, C)), Buf((G, C)), Buf((C,), data=d["rm0"]), Buf((C,), data=d["rv0"]), workspace(R, C, G)
        assert L().dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, None, ws.ptr, R, N, C, G, float(EPSF), float(MOMF), st()) == 0
        o += [mean.bits(), rstd.bits(), rm.bits(), rv.bits()]
        # dvae_bn_stats_finalize on the partials that launch left: the same statistics, the running ones one call further
        mean2, rstd2 = Buf((G, C)), Buf((G, C))
        assert L().dvae_bn_stats_finalize(mean2.ptr, rstd2.ptr, rm.ptr, rv.ptr, None, ws.ptr, R, N, C, G, float(EPSF), float(MOMF), st()) == 0
        guards(mean, rstd, mean2, rstd2, rm, rv, ws)
        assert np.array_equal(mean2.bits(), mean.bits()) and np.array_equal(rstd2.bits(), rstd.bits())
        o += [rm.bits(), rv.bits()]
        z = Buf((R, C))
        apply_fwd(c, z, B.ACT_TANH, c.res)
        o.append(z.bits())
        for from_y, a in ((False, B.ACT_TANH), (True, B.ACT_RELU)):
            dy, dg, db, ws = Buf((R, C)), Buf((C,), data=d["dgamma0"]), Buf((C,), data=d["dbeta0"]), workspace(R, C, G)
            assert launch_bwd(c, a, from_y, z=None if from_y else c.z(a), dy=dy, dgamma=dg, dbeta=db, ws=ws) == 0
            guards(dy, dg, db, ws)
            o += [dy.bits(), dg.bits(), db.bits()]
        out.append(o)
    assert all(np.array_equal(a, b) for a, b in zip(*out))


def test_refusals_change_nothing():
    case = B.CASES[2]
    R, N, G, C = case
    c = ctx(case)
    d = c.d
    z = c.z(B.ACT_RELU)
    mean, rstd, rm, rv = Buf((G, C)), Buf((G, C)), Buf((C,), data=d["rm0"]), Buf((C,), data=d["rv0"])
    nbt, zo, dy, dg, db, ws = (Buf((1,), torch.int64, data=np.array([1], np.int64)), Buf((R, C)), Buf((R, C)), Buf((C,), data=d["dgamma0"]),
                               Buf((C,), data=d["dbeta0"]), workspace(R, C, G))
    outs = (mean, rstd, rm, rv, nbt, zo, dy, dg, db, ws)
    before = [b.bits() for b in outs]
    e, m, s = float(EPSF), float(MOMF), st()
    shapes = {"C % 4": (R, N, C - 1, G), "R % N": (R, N + 1, C, G), "N % G": (R, N, C, 2), "G = 0": (R, N, C, 0), "G = 3": (R + 1, 6, C, 3),
              "R = 0": (0, N, C, G), "C = 0": (R, N, 0, G), "N = 0": (R, 0, C, G)}
    assert (R + 1) % 6 == 0
    lib = L()
    for what, (r, n, cc, g) in shapes.items():
        assert lib.dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, ws.ptr, r, n, cc, g, e, m, s) == EINVAL, what
        assert lib.dvae_bn_stats_finalize(mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, ws.ptr, r, n, cc, g, e, m, s) == EINVAL, what
        assert lib.dvae_bn_apply_fwd(c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, c.beta.ptr, None, zo.ptr, r, n, cc, g, 1, 0, s) == EINVAL, what
        assert lib.dvae_bn_bwd(c.dz.ptr, c.y.ptr, z.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, dy.ptr, dg.ptr, db.ptr, ws.ptr, r, n, cc, g, 1, 0, s) == EINVAL, what
        assert lib.dvae_bn_bwd_from_y(c.dz.ptr, c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, c.beta.ptr, dy.ptr, dg.ptr, db.ptr, ws.ptr,
                                      r, n, cc, g, 1, 0, s) == EINVAL, what
    # null pointers: the workspace of each entry point that has one, beta of bwd_from_y, Z of bwd; tanh without Z
    assert lib.dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, None, R, N, C, G, e, m, s) == EINVAL
    assert lib.dvae_bn_stats_finalize(mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, None, R, N, C, G, e, m, s) == EINVAL
    assert lib.dvae_bn_bwd(c.dz.ptr, c.y.ptr, z.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, dy.ptr, dg.ptr, db.ptr, None, R, N, C, G, 1, 0, s) == EINVAL
    assert lib.dvae_bn_bwd_from_y(c.dz.ptr, c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, c.beta.ptr, dy.ptr, dg.ptr, db.ptr, None,
                                  R, N, C, G, 1, 0, s) == EINVAL
    assert lib.dvae_bn_bwd_from_y(c.dz.ptr, c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, None, dy.ptr, dg.ptr, db.ptr, ws.ptr,
                                  R, N, C, G, 1, 0, s) == EINVAL
    assert lib.dvae_bn_bwd(c.dz.ptr, c.y.ptr, None, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, dy.ptr, dg.ptr, db.ptr, ws.ptr, R, N, C, G, 1, 0, s) == EINVAL
    assert lib.dvae_bn_bwd_from_y(c.dz.ptr, c.y.ptr, c.mean.ptr, c.rstd.ptr, c.gamma.ptr, c.beta.ptr, dy.ptr, dg.ptr, db.ptr, ws.ptr,
                                  R, N, C, G, B.ACT_TANH, 0, s) == EINVAL
    assert lib.dvae_bn_apply_fwd(c.y.ptr, c.mean.ptr, c.rstd.ptr, None, c.beta.ptr, None, zo.ptr, R, N, C, G, 1, 0, s) == EINVAL
    guards(*outs)
    assert all(np.array_equal(a, b.bits()) for a, b in zip(before, outs))
    # ... and a good call is taken
    assert lib.dvae_bn_stats_fwd(c.y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, nbt.ptr, ws.ptr, R, N, C, G, e, m, s) == 0
    assert int(nbt.np()[0]) == 1 + G and np.array_equal(mean.bits(), c.mean.bits())
