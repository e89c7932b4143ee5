"""The latent-report kernels of csrc/latents.hip (dvae_latent_tables, dvae_latent_lse) on the MI355X
through the C ABI, against the float64 restatement of tests/latents_ref.py, and dvae_amd.latents above them.

Every LSE is held to the bound derived in latents_ref (from 2^-24 and the operation counts, not from what the kernel gives)
against float64 on the rounded tables; what the contract calls bit-exact is compared bit for bit: two launches, five jobs in
one launch against five launches, a row alone against the same row among 129 others.  Every buffer a launch may write is a
guarded one of tests/kernel_harness.py, pre-filled with 0xFF; inputs carry NaN wherever the entry point must not read.
The worst error / bound per shape is printed at the module's end.

Worst error / bound on the MI355X, per (D, S, ld): lse 0.486 (1, 0, 1), 0.655 (1, 1, 1), 0.535 (2, 1, 2), 0.628 (5, 2, 7),
0.666 (32, 4, 32), 0.721 (64, 16, 64); tables z 0.986, a 0.775, h 0.672; the planted Gaussian's shared information 0.004 of
its summed bound (1.04e-4 nats), the planted speakers' information 0.001 / 0.005 of theirs; the report's own launches 0.145
(planted) and 0.276 (end to end).
"""
import json
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, F32, F64, guards, ibuf, L, make_trainer, ok, Pad, st, untouched, Worst
import dvae_amd  # noqa: E402,F401
import latents_ref as R  # noqa: E402

WORST = Worst("test_hip_latents.py (rows: D, S, ld)")
note = WORST.note


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


class Tabs:
    """the four tables of a kernel_case on the device, NaN around them and in the columns D .. ld - 1"""

    def __init__(self, case):
        self.z, self.mu, self.a, self.h = (Pad(f) for f in case["full"])

    def bufs(self):
        return [p.buf for p in (self.z, self.mu, self.a, self.h)]


def lse(t, ld, D, S, jobs, rows_out, ldo, jobs_host=None, njobs=None, rc=0, **kw):
    jobs = np.ascontiguousarray(jobs, np.int64).reshape(-1, 5)
    jb = ibuf(jobs)
    out = Buf((rows_out, ldo))
    host = jobs if jobs_host is None else np.ascontiguousarray(jobs_host, np.int64)
    args = dict(z=t.z.ptr, mu=t.mu.ptr, a=t.a.ptr, h=t.h.ptr, ld=ld, D=D, S=S, jobs=jb.ptr, host=host.ctypes.data,
                njobs=len(jobs) if njobs is None else njobs, out=out.ptr, ldo=ldo)
    args.update(kw)
    got = L().dvae_latent_lse(args["z"], args["mu"], args["a"], args["h"], args["ld"], args["D"], args["S"], args["jobs"],
                              args["host"], args["njobs"], args["out"], args["ldo"], st())
    if rc == 0:
        ok(got, "dvae_latent_lse")
    else:
        assert got == rc, got
    guards(out, jb, *t.bufs())
    return out


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("ncols", R.NCOLS)
@pytest.mark.parametrize("D,S,ld", R.SHAPES)
def test_lse_against_float64(D, S, ld, ncols):
    """one launch of four jobs, nrows = 1, 64, 65, 130 from the same first row against the same columns"""
    c = R.kernel_case(D, S, ld, ncols)
    t = Tabs(c)
    ldo = D + 5
    out0 = np.concatenate([[0], np.cumsum(R.NROWS)[:-1]]) + 2
    jobs = [[R.ROW0, n, R.COL0, ncols, o] for n, o in zip(R.NROWS, out0)]
    total = int(out0[-1] + R.NROWS[-1]) + 1
    out = lse(t, ld, D, S, jobs, total, ldo)
    got, gb = out.np(), out.bits()
    L64, B = R.lse_tables(*(c[k].astype(F64) for k in ("z", "mu", "a", "h")), S, (R.ROW0, 130), (R.COL0, ncols), bound=True)
    key = f"{D},{S},{ld}"
    untouched(gb[:, D + 3:], "the columns behind D + 3")
    untouched(gb[:2], "the rows in front of the first job")
    untouched(gb[total - 1:], "the row behind the last job")
    for n, o in zip(R.NROWS, out0):
        g_ = got[o:o + n, :D + 3]
        assert np.all(np.isfinite(g_)), "a row far from every column must stay finite"
        note((key, "lse"), g_, L64[:n], B[:n], f"ncols={ncols} nrows={n}")
        assert np.array_equal(gb[o:o + n, :D + 3], gb[out0[-1]:out0[-1] + n, :D + 3]), "a row does not depend on the job's other rows"
    assert L64[0, D + 2] < -1e3 * D and L64[1, D + 2] < -1e6 * D                      # the far rows are far
    out2 = lse(t, ld, D, S, jobs, total, ldo)
    assert np.array_equal(out2.bits(), gb), "a second launch gives the same bits"


# ----------------------------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("D,S,ld", [(5, 2, 7), (32, 4, 32)])
def test_jobs_in_one_launch_and_alone(D, S, ld):
    c = R.kernel_case(D, S, ld, 257)
    t = Tabs(c)
    ldo = D + 3
    jobs = np.array([[R.ROW0, 130, R.COL0, 257, 0], [0, 65, 0, 100, 130], [10, 0, 0, 5, 195], [7, 1, 200, 1, 195],
                     [40, 64, R.COL0 + 3, 63, 196]], np.int64)
    total = 260
    both = lse(t, ld, D, S, jobs, total, ldo).bits()
    for k, j in enumerate(jobs):
        alone = lse(t, ld, D, S, j[None], total, ldo).bits()
        r0, n = int(j[4]), int(j[1])
        assert np.array_equal(alone[r0:r0 + n], both[r0:r0 + n]), f"job {k}: alone and among five"
        untouched(alone[:r0], f"job {k}: rows in front")
        untouched(alone[r0 + n:], f"job {k}: rows behind")
    # a row alone against the same row among 129 others
    for r in (0, 1, 64, 129):
        one = lse(t, ld, D, S, [[R.ROW0 + r, 1, R.COL0, 257, 0]], 1, ldo).bits()
        assert np.array_equal(one[0], both[r]), f"row {r}: alone and among 130"


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched():
    D, S, ld = 5, 2, 7
    c = R.kernel_case(D, S, ld, 65)
    t = Tabs(c)
    good = np.array([[R.ROW0, 10, R.COL0, 65, 0]], np.int64)
    big = Tabs(R.kernel_case(64, 16, 80, 2))

    def refused(jobs=good, **kw):
        out = lse(t, kw.pop("ld", ld), kw.pop("D", D), kw.pop("S", S), jobs, 12, kw.pop("ldo", 8), rc=EINVAL, **kw)
        assert out.poisoned().all(), "a refused call wrote an output"

    for kw in (dict(z=None), dict(mu=None), dict(a=None), dict(h=None), dict(jobs=None), dict(host=None), dict(out=None),
               dict(njobs=0), dict(njobs=-1), dict(D=0), dict(S=-1), dict(S=6), dict(ld=4), dict(ldo=7),
               dict(D=65, ld=80, ldo=80, z=big.z.ptr, mu=big.mu.ptr, a=big.a.ptr, h=big.h.ptr)):
        if "jobs" in kw and kw["jobs"] is None:
            out = Buf((12, 8))
            rc = L().dvae_latent_lse(t.z.ptr, t.mu.ptr, t.a.ptr, t.h.ptr, ld, D, S, None, good.ctypes.data, 1, out.ptr, 8, st())
            assert rc == EINVAL and out.poisoned().all()
            continue
        refused(**kw)
    for bad in ([[-1, 10, 0, 65, 0]], [[0, -1, 0, 65, 0]], [[0, 10, -1, 65, 0]], [[0, 10, 0, 0, 0]], [[0, 10, 0, -3, 0]],
                [[0, 10, 0, 65, -1]], [[0, 0, 0, 0, 0]]):
        refused(jobs=np.array(bad, np.int64))
    # a good job in front of a bad one: nothing is launched
    refused(jobs=np.array([[R.ROW0, 10, R.COL0, 65, 0], [0, 1, 0, 0, 11]], np.int64))
    # a misaligned job table
    jb = ibuf(np.concatenate([[0], good.reshape(-1)]))
    out = Buf((12, 8))
    rc = L().dvae_latent_lse(t.z.ptr, t.mu.ptr, t.a.ptr, t.h.ptr, ld, D, S, jb.at(0) + 4, good.ctypes.data, 1, out.ptr, 8, st())
    assert rc == EINVAL and out.poisoned().all()
    # nrows = 0 is a no-op, alone and beside a job that has rows
    out = lse(t, ld, D, S, [[R.ROW0, 0, R.COL0, 65, 0]], 12, 8)
    assert out.poisoned().all()
    out = lse(t, ld, D, S, [[R.ROW0, 0, R.COL0, 65, 0], [R.ROW0, 2, R.COL0, 65, 3]], 12, 8)
    p = out.poisoned()
    assert p[:3].all() and p[5:].all() and not p[3:5, :8].any()


# ---------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("N,D,ld", [(1, 1, 1), (257, 5, 7), (1000, 32, 33), (130, 64, 64)])
def test_tables_elementwise(N, D, ld):
    rs = np.random.RandomState(N + D)
    mu, eps = rs.randn(N, D).astype(F32), rs.randn(N, D).astype(F32)
    lv = rs.uniform(-6.0, 2.0, (N, D)).astype(F32)
    lv.reshape(-1)[::7] = -20.0
    lv.reshape(-1)[3::11] = 10.0

    def wide(v):
        f = np.full((N, ld), np.nan, F32)
        f[:, :D] = v
        return Pad(f)

    pm, pl, pe = wide(mu), wide(lv), wide(eps)
    z, a, h = Buf((N, ld)), Buf((N, ld)), Buf((N, ld))
    ok(L().dvae_latent_tables(pm.ptr, pl.ptr, pe.ptr, z.ptr, a.ptr, h.ptr, N, D, ld, st()), "dvae_latent_tables")
    guards(z, a, h, pm.buf, pl.buf, pe.buf)
    z64, _, a64, h64 = R.tables(mu, lv, eps, dtype=F64)
    bz, ba, bh = R.tables_bound(mu, lv, eps)
    key = f"tables {D},{ld}"
    for name, buf, ref, b in (("z", z, z64, bz), ("a", a, a64, ba), ("h", h, h64, bh)):
        note((key, name), buf.np()[:, :D], ref, b, f"{name} N={N}")
        untouched(buf.bits()[:, D:], f"{name}: the columns behind D")
    # refusals write nothing; N = 0 is a no-op
    for kw in (dict(D=0), dict(D=65), dict(ld=D - 1), dict(N=-1), dict(mu=None), dict(z=None)):
        a_ = dict(mu=pm.ptr, lv=pl.ptr, eps=pe.ptr, z=True, N=N, D=D, ld=ld)
        a_.update(kw)
        o = [Buf((N, ld)) for _ in range(3)]
        rc = L().dvae_latent_tables(a_["mu"], a_["lv"], a_["eps"], o[0].ptr if a_["z"] else None, o[1].ptr, o[2].ptr, a_["N"],
                                    a_["D"], a_["ld"], st())
        assert rc == EINVAL and all(b.poisoned().all() for b in o), kw
    o = [Buf((N, ld)) for _ in range(3)]
    ok(L().dvae_latent_tables(pm.ptr, pl.ptr, pe.ptr, o[0].ptr, o[1].ptr, o[2].ptr, 0, D, ld, st()))
    assert all(b.poisoned().all() for b in o)


# ------------------------------------------------------------------------------------------------ the planted cases
def gpu_report(p, seed=0):
    from dvae_amd import latents
    return latents.LatentReport("cuda").report(p["mu"], p["lv"], p["speakers"], p["S"], seed=seed, eps=p["eps"])


def reference_on(res, p):
    """float64 on the GPU's own tables (as rounded they are the model) -> (quantities, L_all, B_all, L_own, B_own)"""
    z, mu, a, h = (res["_tables"][k].astype(F64) for k in ("z", "mu", "a", "h"))
    N = len(z)
    L_all, B_all = R.lse_tables(z, mu, a, h, p["S"], (0, N), (0, N), bound=True)
    own = [R.lse_tables(z, mu, a, h, p["S"], (r0, n), (r0, n), bound=True) for r0, n in R.speaker_jobs(p["speakers"])]
    L_own, B_own = np.concatenate([o[0] for o in own]), np.concatenate([o[1] for o in own])
    return R.quantities(z, mu, a, h, p["S"], p["speakers"], L_all, L_own), L_all, B_all, L_own, B_own


def test_planted_gaussian_on_the_gpu():
    p = R.planted_gaussian(0)
    res = gpu_report(p)
    ref, L_all, B_all, _, _ = reference_on(res, p)
    D = 2
    bound = float(np.mean(B_all[:, D] + B_all[:, D + 1] + B_all[:, D + 2]))
    print(f"shared {res['shared']!r}, float64 {ref['shared']!r}, bound {bound:.3g}")
    assert 0.2 > 1000.0 * bound, bound
    assert 0.22 <= res["shared"] <= 0.31
    assert abs(res["shared"] - ref["shared"]) <= bound
    WORST.record(("planted", "shared"), abs(res["shared"] - ref["shared"]) / bound)
    note(("planted", "lse"), res["_lse"][:len(L_all)], L_all, B_all, "the global job of the planted Gaussian")
    for seed in (1, 2):
        assert 0.22 <= gpu_report(R.planted_gaussian(seed))["shared"] <= 0.31
    for seed in (0, 1, 2):
        assert abs(gpu_report(R.planted_gaussian(seed, independent=True))["shared"]) <= 0.01


def test_planted_speakers_on_the_gpu():
    p = R.planted_speakers(0)
    res = gpu_report(p)
    ref, L_all, B_all, L_own, B_own = reference_on(res, p)
    D, N = 5, len(L_all)
    assert abs(res["speaker_entropy"] - math.log(4)) <= 1e-12 and res["small_speakers"] == [] and res["non_finite_chunks"] == []
    for name, col in (("style", D), ("content", D + 1)):
        bound = float(np.mean(B_all[:, col] + B_own[:, col]))
        got, want = res["speaker_info"][name], ref["speaker_info_" + name]
        print(f"speaker information {name}: {got!r}, float64 {want!r}, bound {bound:.3g}")
        assert 0.2 > 1000.0 * bound, bound
        assert abs(got - want) <= bound
        WORST.record(("planted", "speaker " + name), abs(got - want) / bound)
    assert abs(res["speaker_info"]["style"] - math.log(4)) <= 0.01 and res["speaker_info"]["content"] < 0.1
    note(("planted", "lse"), res["_lse"][N:], L_own, B_own, "the speakers' jobs")
    for name in ("style", "content", "joint"):
        b = res["blocks"][name]
        assert abs(b["mi"] + b["tc"] + b["dwkl"] - b["kl_sample"]) <= 1e-10
        assert b["mi"] <= math.log(N) + 1e-3
    for seed in (1, 2):
        r = gpu_report(R.planted_speakers(seed))
        assert abs(r["speaker_info"]["style"] - math.log(4)) <= 0.01 and r["speaker_info"]["content"] < 0.1


def test_non_finite_chunks_are_compacted_out():
    p = R.planted_speakers(1, per=16)
    keep = np.ones(64, bool)
    keep[[5, 40]] = False
    mu = p["mu"].copy()
    mu[5, 1], lv = np.nan, p["lv"].copy()
    lv[40, 3] = np.inf
    res = gpu_report(dict(p, mu=mu, lv=lv))
    clean = gpu_report({k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in p.items()})
    assert res["non_finite_chunks"] == [5, 40] and res["n_chunks"] == 62
    assert res["shared"] == clean["shared"] and res["speaker_info"] == clean["speaker_info"] and res["blocks"] == clean["blocks"]


# --------------------------------------------------------------------------------------------------------- end to end
def test_cli_end_to_end(tmp_path, capsys):
    from dvae_amd import latents
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=3, n_utt=4, length=130)
    run_dir = tmp_path / "run"
    (run_dir / "checkpoints").mkdir(parents=True)
    cfg = dict(samples_length=64, latent_size=32, speaker_size=4, lr=1e-4, batch_size=4, mse_cof=10, kl_cof=10)
    (run_dir / "config.json").write_text(json.dumps(cfg))
    w = make_trainer(batch=4, n_frames=64)
    torch.save(w.model.state_dict(), run_dir / "checkpoints" / "DisentangledVAE_VCTK_2.pth")
    argv = [corpus, "--log_dir", str(run_dir), "--seed", "3"]
    assert latents.main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    first = (run_dir / "latents.json").read_bytes()
    res = json.loads(first)
    assert res["lines"] == out[:len(res["lines"])] and res["n_chunks"] == 24 and res["checkpoint_epoch"] == 2
    assert res["speaker_chunks"] == {"spk000": 8, "spk001": 8, "spk002": 8} and res["small_speakers"] == []
    num = r"(-?[0-9.e+-]+|nan|inf)"
    for name in ("style", "content", "joint"):
        m = re.match(rf"^latents {name}: kl {num} nats, active units (\d+)/(\d+), mi {num} \(ln N = {num}\), tc {num}, "
                     rf"dwkl {num}$", out[("style", "content", "joint").index(name)])
        assert m, out[:3]
        b = res["blocks"][name]
        assert [float(m.group(i)) for i in (1, 4, 5, 6, 7)] == [b["kl"], b["mi"], res["ln_n"], b["tc"], b["dwkl"]]
        assert (int(m.group(2)), int(m.group(3))) == (b["active_units"], b["dims"])
    assert res["ln_n"] == math.log(24) and res["blocks"]["style"]["dims"] == 4 and res["blocks"]["content"]["dims"] == 28
    assert out[3] == f"style/content shared information: {res['shared']} nats"
    assert out[4] == (f"speaker information: style {res['speaker_info']['style']}, content {res['speaker_info']['content']} "
                      f"of H = {res['speaker_entropy']} nats")
    assert len([l for l in out if l.startswith("dimension ") and l.split()[1].isdigit()]) == 32 == len(res["dimensions"])
    # the same figures from the pieces, and float64 on the downloaded tables within the bounds
    chunks = latents.list_chunks(corpus, 64)
    mu, lv = latents.encode_posteriors(w, chunks)
    rep = latents.LatentReport("cuda").report(mu, lv, chunks.speaker, 4, seed=3)
    assert rep["shared"] == res["shared"] and rep["blocks"] == res["blocks"] and rep["speaker_info"] == res["speaker_info"]
    p = dict(S=4, speakers=chunks.speaker)
    ref, L_all, B_all, L_own, B_own = reference_on(rep, p)
    note(("cli", "lse"), rep["_lse"], np.concatenate([L_all, L_own]), np.concatenate([B_all, B_own]), "the report's launch")
    D = 32
    assert abs(res["shared"] - ref["shared"]) <= float(np.mean(B_all[:, D:].sum(1)))
    for name, col in (("style", D), ("content", D + 1), ("joint", D + 2)):
        assert abs(res["blocks"][name]["mi"] - ref[name]["mi"]) <= float(np.mean(B_all[:, col])) + 1e-12
        sl = slice(0, 4) if name == "style" else slice(4, D) if name == "content" else slice(0, D)
        assert abs(res["blocks"][name]["tc"] - ref[name]["tc"]) <= float(np.mean(B_all[:, col] + B_all[:, sl].sum(1))) + 1e-12
        assert abs(res["blocks"][name]["dwkl"] - ref[name]["dwkl"]) <= float(np.mean(B_all[:, sl].sum(1))) + 1e-12
    for name, col in (("style", D), ("content", D + 1)):
        assert abs(res["speaker_info"][name] - ref["speaker_info_" + name]) <= float(np.mean(B_all[:, col] + B_own[:, col]))
    st_ = R.host_stats(rep["_tables"]["mu"], lv.cpu().numpy(), 4)
    assert np.allclose([d["kl"] for d in res["dimensions"]], st_["kl"], rtol=1e-12, atol=0)
    assert [d["active"] for d in res["dimensions"]] == st_["active"].tolist()
    # a second run is byte-identical
    assert latents.main(argv) == 0
    capsys.readouterr()
    assert (run_dir / "latents.json").read_bytes() == first
