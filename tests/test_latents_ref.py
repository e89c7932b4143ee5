"""The float64 restatement of the latent report (tests/latents_ref.py) on the CPU: closed forms, the
planted Gaussian and the planted speakers, the fp32 walk in the kernel's order inside the derived bounds on every shape of
tests/test_hip_latents.py, and the plumbing (header, binding, ABI number, command-line errors)."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import latents_ref as R  # noqa: E402
from ref_common import F, F64, fma, worst_ratio  # noqa: E402


@pytest.fixture(scope="module")
def gaussian():
    return {(seed, ind): R.report(**{k: v for k, v in R.planted_gaussian(seed, ind).items()})
            for seed in (0, 1, 2) for ind in (False, True)}


@pytest.fixture(scope="module")
def speakers():
    return {seed: R.report(**R.planted_speakers(seed)) for seed in (0, 1, 2)}


# -------------------------------------------------------------------------------------------------------- closed forms
def test_identical_posteriors_carry_nothing():
    N, D, S = 64, 5, 2
    rs = np.random.RandomState(0)
    mu, lv = np.tile(rs.randn(1, D), (N, 1)), np.tile(rs.uniform(-1, 1, (1, D)), (N, 1))
    r = R.report(mu, lv, rs.randn(N, D), np.zeros(N, np.int32), S, dtype=F64)
    for v in (r["joint"]["mi"], r["joint"]["tc"], r["style"]["mi"], r["content"]["tc"], r["shared"]):
        assert abs(v) <= 1e-12, v


def test_far_apart_posteriors_carry_ln_n():
    N, D, S = 64, 3, 1
    rs = np.random.RandomState(1)
    mu = 1000.0 * np.arange(N)[:, None] * np.ones((1, D))
    r = R.report(mu, np.zeros((N, D)), rs.randn(N, D), np.zeros(N, np.int32), S, dtype=F64)
    assert abs(r["joint"]["mi"] - math.log(N)) <= 1e-9 and abs(r["style"]["mi"] - math.log(N)) <= 1e-9


@pytest.mark.parametrize("S", [0, 2, 5])
def test_decomposition_identity(S):
    N, D = 200, 5
    rs = np.random.RandomState(2)
    r = R.report(rs.randn(N, D), rs.uniform(-3, 1, (N, D)), rs.randn(N, D), np.repeat(np.arange(4), 50), S)
    for name in ("style", "content", "joint"):
        b = r[name]
        assert abs(b["mi"] + b["tc"] + b["dwkl"] - b["kl_sample"]) <= 1e-10, name
    empty = "style" if S == 0 else "content" if S == D else None
    if empty:
        assert all(abs(v) <= 1e-12 for v in r[empty].values()), r[empty]      # an empty block's LSE is ln N
        assert abs(r["shared"]) <= 1e-12


def test_empty_block_lse_is_ln_cols():
    c = R.kernel_case(5, 0, 7, 65)
    L = R.lse_tables(c["z"].astype(F64), c["mu"].astype(F64), c["a"].astype(F64), c["h"].astype(F64), 0, (R.ROW0, 4),
                     (R.COL0, 65))
    assert np.all(np.abs(L[:, 5] - math.log(65)) <= 1e-14) and np.array_equal(L[:, 6], L[:, 7])


# ---------------------------------------------------------------------------------------------------- planted Gaussian
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_gaussian_shares_what_the_correlation_says(gaussian, seed):
    shared = gaussian[(seed, False)]["shared"]
    print(f"seed {seed}: shared {shared:.4f} (N -> inf: {-0.5 * math.log(1 - 0.64 ** 2):.4f})")
    assert 0.22 <= shared <= 0.31


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_gaussian_independent_blocks_share_nothing(gaussian, seed):
    shared = gaussian[(seed, True)]["shared"]
    print(f"seed {seed}: shared {shared:.4f}")
    assert abs(shared) <= 0.01


# ---------------------------------------------------------------------------------------------------- planted speakers
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_speakers(speakers, seed):
    r = speakers[seed]
    print(f"seed {seed}: style {r['speaker_info_style']:.5f}, content {r['speaker_info_content']:.5f}, H {r['speaker_entropy']:.5f}")
    assert abs(r["speaker_entropy"] - math.log(4)) <= 1e-12
    assert abs(r["speaker_info_style"] - math.log(4)) <= 0.01
    assert r["speaker_info_content"] < 0.1


def test_small_speakers_are_left_out_and_runs_are_found():
    spk = np.array([0] * 9 + [1] * 3 + [2] * 8)
    assert R.speaker_jobs(spk) == [(0, 9), (9, 3), (12, 8)]
    rs = np.random.RandomState(3)
    mu, lv, eps = rs.randn(20, 2), np.zeros((20, 2)), rs.randn(20, 2)
    r = R.report(mu, lv, eps, spk, 1)
    keep = np.r_[0:9, 12:20]
    L_all, L_own, D = r["L_all"], r["L_own"], 2
    ng = np.r_[[9.0] * 9, [8.0] * 8]
    ref = np.mean((L_own[keep, D] - np.log(ng)) - (L_all[keep, D] - math.log(20)))
    assert abs(r["speaker_info_style"] - ref) <= 1e-14


def test_host_stats():
    rs = np.random.RandomState(4)
    mu = rs.randn(500, 4) * np.array([1.0, 0.05, 0.5, 0.01])
    st = R.host_stats(mu, np.zeros((500, 4)), 2)
    assert st["active"].tolist() == [True, False, True, False]
    assert np.allclose(st["kl"], 0.5 * (mu * mu).mean(0), rtol=1e-12) and np.allclose(st["mean_var"], 1.0)


# -------------------------------------------------------------------------------------------------------------- bounds
def test_quarters_partition_every_column_once():
    for n in R.NCOLS + [3, 4, 5, 7]:
        qs = R.quarters(n)
        assert qs[0][0] == 0 and qs[-1][1] == n and all(a[1] == b[0] for a, b in zip(qs, qs[1:]))
        assert all(c1 > c0 for c0, c1 in qs) and len(qs) == min(4, -(-n // -(-n // 4)))


@pytest.mark.parametrize("D,S,ld", R.SHAPES)
def test_fp32_walk_in_the_kernels_order_stays_inside_the_bounds(D, S, ld):
    """every (ncols, shape) of the GPU suite, on its 130 rows (the smaller row counts are prefixes of them)"""
    worst = 0.0
    for ncols in R.NCOLS:
        c = R.kernel_case(D, S, ld, ncols)
        rows, cols = (R.ROW0, 130), (R.COL0, ncols)
        L, B = R.lse_tables(*(c[k].astype(F64) for k in ("z", "mu", "a", "h")), S, rows, cols, bound=True)
        got = R.lse_f32(c["z"], c["mu"], c["a"], c["h"], S, rows, cols)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(B)) and np.all(B > 0)
        ratio, at = worst_ratio(got, L, B)
        assert ratio <= 1.0, (ncols, at, ratio)
        worst = max(worst, ratio)
        # the bound is not vacuous where it matters: an ordinary row's is far below a hundredth of a nat
        assert np.median(B[2:]) < 1e-3 * max(1.0, np.median(np.abs(L[2:]))), (ncols, np.median(B[2:]))
    print(f"D {D}, S {S}: worst error / bound of the fp32 walk {worst:.3f}")


def test_tables_bound_holds_for_an_fp32_evaluation():
    rs = np.random.RandomState(6)
    mu, lv, eps = (v.astype(F) for v in (rs.randn(300, 5), rs.uniform(-20, 10, (300, 5)), rs.randn(300, 5)))
    z64, _, a64, h64 = R.tables(mu, lv, eps, dtype=F64)
    bz, ba, bh = R.tables_bound(mu, lv, eps)
    # the kernel's roundings with an exponential rounded once (numpy's fp32 exp is allowed more than the 1 ulp of the
    # device library's, so it is not the stand-in here)
    z = fma(np.exp(0.5 * lv.astype(F64)).astype(F), eps, mu)
    a = -(F(R.HALF_LOG_2PI) + F(0.5) * lv).astype(F)
    h = (F(0.5) * np.exp(-lv.astype(F64)).astype(F)).astype(F)
    rz, ra, rh = worst_ratio(z, z64, bz)[0], worst_ratio(a, a64, ba)[0], worst_ratio(h, h64, bh)[0]
    print(f"error / bound: z {rz:.3f}, a {ra:.3f}, h {rh:.3f}")
    assert max(rz, ra, rh) <= 1.0 and min(rz, ra, rh) > 0.05      # held, and not by a bound a hundred times too wide


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_header_and_binding_agree():
    from dvae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    assert int(re.search(r"#define DVAE_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 319
    assert int(re.search(r"#define DVAE_LATENT_MAX_D (\d+)", hdr).group(1)) == R.MAX_D == 64
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("dvae_latent_tables", "dvae_latent_lse"):
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    src = open(os.path.join(ROOT, "disentangle-vae-for-vc_amd", "csrc", "latents.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and '#include "latents.hip"' in open(
        os.path.join(ROOT, "disentangle-vae-for-vc_amd", "csrc", "probe.hip")).read()


def test_module_constants_follow_the_reference():
    from dvae_amd import latents
    assert (latents.MAX_D, latents.ACTIVE_VAR, latents.MIN_SPEAKER_CHUNKS) == (R.MAX_D, R.ACTIVE_VAR, R.MIN_SPEAKER_CHUNKS)
    spk = np.array([0] * 9 + [1] * 3 + [4] * 8)
    assert [(r, n) for _, r, n in latents.speaker_runs(spk)] == R.speaker_jobs(spk)
    rs = np.random.RandomState(8)
    # the product's host arithmetic against the reference's, on the reference's own LSE tables
    p = R.planted_speakers(0, per=16)
    ref = R.report(**p)
    z, mu, a, h = ref["tables"]
    got = latents.quantities(dict(z=z, mu=mu, a=a, h=h), p["lv"], ref["L_all"], ref["L_own"], p["speakers"], p["S"])
    for name in ("style", "content", "joint"):
        for k in ("mi", "tc", "dwkl"):
            assert abs(got["blocks"][name][k] - ref[name][k]) <= 1e-12, (name, k)
    assert abs(got["shared"] - ref["shared"]) <= 1e-12 and abs(got["speaker_entropy"] - ref["speaker_entropy"]) <= 1e-12
    assert abs(got["speaker_info"]["style"] - ref["speaker_info_style"]) <= 1e-12
    st = R.host_stats(mu, p["lv"], p["S"])
    assert np.allclose([d["kl"] for d in got["dimensions"]], st["kl"], rtol=1e-12)
    assert [d["active"] for d in got["dimensions"]] == st["active"].tolist()
    assert got["blocks"]["style"]["active_units"] == int(st["active"][:2].sum())
    del rs


def test_subset_keeps_the_order():
    from dvae_amd import latents, probe
    ch = probe.Chunks(n_frames=64, speakers=["a"], utterances=[], utt=np.arange(100), start=np.zeros(100, np.int64),
                      speaker=np.zeros(100, np.int32), held_out=np.zeros(100, bool))
    idx = latents.subset(ch, 10, 3)
    assert len(idx) == 10 and np.all(np.diff(idx) > 0) and np.array_equal(idx, latents.subset(ch, 10, 3))
    assert np.array_equal(latents.subset(ch, 100, 3), np.arange(100)) and not np.array_equal(idx, latents.subset(ch, 10, 4))


def test_cli_argument_errors_return_2(tmp_path, capsys):
    from dvae_amd import latents
    assert latents.main([]) == 2
    assert latents.main([str(tmp_path)]) == 2                                         # no --log_dir
    assert latents.main([str(tmp_path), "--log_dir", str(tmp_path), "--no-such-flag"]) == 2
    assert latents.main([str(tmp_path), "--log_dir", str(tmp_path)]) == 2             # no config.json
    (tmp_path / "config.json").write_text("{}")
    assert latents.main([str(tmp_path / "nowhere"), "--log_dir", str(tmp_path)]) == 2
    assert latents.main([str(tmp_path), "--log_dir", str(tmp_path), "--max-chunks", "0"]) == 2
    assert latents.main([str(tmp_path), "--log_dir", str(tmp_path)]) == 1             # no checkpoint: not an argument error
    assert "latents:" in capsys.readouterr().err
