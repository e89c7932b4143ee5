"""CPU checks of the GMM-UBM speaker verification: the float64 restatement tests/gmm_ref.py holds
the properties the GPU suite builds on (EM ascends, MAP's limits, the planted speakers are separable by a margin no
rounding can turn, the fp32 walk stays inside the derived bounds), and dvae_amd.verify's host logic agrees with it."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (3, 23), (64, 23), (256, 32), (5, 7)]          # (K, D) of the GPU suite


def planted_mixture(seed, K=4, D=3, N=400):
    rs = np.random.RandomState(seed)
    c = rs.randn(K, D) * 3.0
    return c[rs.randint(0, K, N)] + rs.randn(N, D) * rs.uniform(0.3, 1.0, (1, D))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_em_ascends(seed):
    x = planted_mixture(seed)
    w, mu, var, _ = G.init_from_frames(x, 4, seed)
    _, _, _, lls = G.em(x, w, mu, var, 10, dtype=np.float64)
    assert len(lls) == 10 and np.all(np.isfinite(lls))
    assert np.min(np.diff(lls)) >= -1e-12, np.diff(lls)


def planted_pipeline(seed=0, K=8, iters=10):
    p = G.planted_speakers(seed)
    x = np.concatenate(p["train"])
    w, mu, var, _ = G.init_from_frames(x, K, 0)
    w, mu, var, lls = G.em(x, w, mu, var, iters)
    ubm = (w, mu, var)
    models = []
    for xs in p["train"]:
        n, f, _ = G.stats(xs, G.loglik(xs, *G.tables(*ubm))[2])
        models.append(G.map_adapt(w, mu, var, n, f, len(xs)))
    return p, ubm, models


def margin_and_bound(segments, ubm, models, D):
    """the smallest (own speaker's llr - the other's) over the segments, and the largest lse bound of their frames under
    any of the three models"""
    gaps, worst = [], 0.0
    for sp, seg in segments:
        sc = [G.llr(seg, m, ubm) for m in models]
        gaps.append(sc[sp] - sc[1 - sp])
        for m in models + [ubm]:
            t = G.tables(*m)
            _, _, g, q = G.loglik(seg, *t)
            worst = max(worst, float(G.lse_bound(t[0], g, q, D).max()))
    return min(gaps), worst


def test_map_limits():
    p, (w, mu, var), _ = planted_pipeline()
    xs = p["train"][0]
    gamma = G.loglik(xs, *G.tables(w, mu, var))[2]
    n, f, _ = G.stats(xs, gamma)
    w2, mu2, var2 = G.map_adapt(w, mu, var, n, f, len(xs), relevance=np.inf)
    assert np.array_equal(w2, w) and np.array_equal(mu2, mu) and np.array_equal(var2, var)
    w0, mu0, var0 = G.map_adapt(w, mu, var, n, f, len(xs), relevance=0.0)
    assert np.all(n > 0)
    assert np.array_equal(mu0, f / n[:, None]) and np.array_equal(var0, var)
    assert np.allclose(w0, n / len(xs), rtol=1e-12, atol=0) and abs(w0.sum() - w.sum()) <= 1e-15


def test_planted_speakers_are_separable_by_a_margin_no_rounding_turns():
    p, ubm, models = planted_pipeline()
    assert len(p["test"]) == 12 and all(seg.shape == (50, 5) for _, seg in p["test"])
    gap, bound = margin_and_bound(p["test"], ubm, models, 5)
    print(f"\nplanted speakers: smallest gap {gap:.4f} nats per frame, largest lse bound {bound:.3g}")
    assert gap > 0, "the float64 pipeline itself misses a segment"
    assert gap > 1000 * bound, (gap, bound)


def test_means_only_adaptation_is_not_enough_here():
    """what DESIGN.md says of means-only MAP on few speakers: the margin collapses (the reason weights are adapted too)"""
    p, ubm, models = planted_pipeline()
    means_only = [(ubm[0], m[1], m[2]) for m in models]
    gap_full, _ = margin_and_bound(p["test"], ubm, models, 5)
    gap_means, _ = margin_and_bound(p["test"], ubm, means_only, 5)
    assert gap_means < 0.25 * gap_full, (gap_means, gap_full)


@pytest.mark.parametrize("K,D", SHAPES)
def test_fp32_walk_stays_six_times_inside_the_bounds(K, D):
    rs = np.random.RandomState(K * 100 + D)
    N = 257
    mu, var = rs.randn(K, D), rs.uniform(0.3, 2.0, (K, D))
    w = rs.dirichlet(np.ones(K))
    if K > 1:
        w = np.maximum(w, 1e-6)
        w[0] = 1e-6
        w /= w.sum()
    x = (mu[rs.randint(0, K, N)] + rs.randn(N, D) * np.sqrt(var.mean())).astype(np.float32)
    x[0] += 50.0
    x[1] += 300.0
    t = G.tables(w, mu, var)
    _, lse, g, q = G.loglik(x, *t)
    _, lse32, g32 = G.loglik_f32(x, *t)
    assert np.all(np.isfinite(lse32)) and lse[1] < -1e4
    r_lse = float((np.abs(lse32 - lse) / G.lse_bound(t[0], g, q, D)).max())
    r_g = float((np.abs(g32 - g) / G.gamma_bound(t[0], g, q, D)).max())
    assert r_lse <= 1 / 6 and r_g <= 1 / 6, (r_lse, r_g)
    assert np.all(np.abs(g32.astype(np.float64).sum(axis=1) - 1.0) <= K * 2.0 ** -23)


def test_score_order_sum_is_a_sum():
    rs = np.random.RandomState(0)
    for n in (0, 1, 63, 256, 257, 1000):
        v = rs.randn(n).astype(np.float32) * 50
        s = G.score_order_sum(v)
        assert abs(s - v.astype(np.float64).sum()) <= (n + 2) * 2.0 ** -53 * np.abs(v).sum()
    assert G.score_order_sum(np.zeros(0, np.float32)) == 0.0


# ------------------------------------------------------------------------------------------------- dvae_amd.verify, host
@pytest.fixture(scope="module")
def vf():
    from dvae_amd import verify
    return verify


def random_model(vf, K=6, D=4, seed=0):
    rs = np.random.RandomState(seed)
    return vf.DiagGMM(rs.dirichlet(np.ones(K)), rs.randn(K, D), rs.uniform(0.2, 3.0, (K, D)))


def test_tables_agree_with_the_reference(vf):
    m = random_model(vf)
    for got, ref in zip(m.tables(), G.tables(m.w, m.mu, m.var)):
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_npz_round_trip_is_bit_equal_and_holds_only_arrays(vf, tmp_path):
    m = random_model(vf, seed=1)
    path = tmp_path / "ubm.npz"
    m.save(path)
    back = vf.DiagGMM.load(path)
    for a, b in ((m.w, back.w), (m.mu, back.mu), (m.var, back.var)):
        assert a.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    with np.load(path, allow_pickle=False) as z:
        assert set(z.files) == {"w", "mu", "var"} | set(vf.FEATURE_CONSTANTS)
        assert z["dim"].item() == 23 and z["col0"].item() == 1
    with np.load(path) as z:
        other = {k: z[k] for k in z.files}
    other["order"] = np.asarray(24)
    with open(tmp_path / "other.npz", "wb") as f:
        np.savez(f, **other)
    with pytest.raises(ValueError, match="other features"):
        vf.DiagGMM.load(tmp_path / "other.npz")


def test_model_limits_are_refused(vf):
    with pytest.raises(ValueError):
        vf.DiagGMM(np.ones(257) / 257, np.zeros((257, 2)), np.ones((257, 2)))
    with pytest.raises(ValueError):
        vf.DiagGMM(np.ones(2) / 2, np.zeros((2, 33)), np.ones((2, 33)))
    with pytest.raises(ValueError):
        vf.DiagGMM(np.ones(2) / 2, np.zeros((2, 3)), np.zeros((2, 3)))


def test_init_is_determined_by_the_seed(vf):
    a, b, c = vf.init_indices(1000, 16, 3), vf.init_indices(1000, 16, 3), vf.init_indices(1000, 16, 4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert len(set(a.tolist())) == 16 and a.min() >= 0 and a.max() < 1000
    x = np.random.RandomState(0).randn(1000, 3)
    w, mu, var, idx = G.init_from_frames(x, 16, 3)
    assert np.array_equal(idx, a)
    m = vf.initial_model(x[a], G.global_variance(x))
    assert np.array_equal(m.w, w) and np.array_equal(m.mu, mu) and np.array_equal(m.var, var)
    with pytest.raises(ValueError):
        vf.init_indices(5, 6, 0)


def test_m_step_floors_and_the_starved_component(vf):
    rs = np.random.RandomState(2)
    K, D, N = 5, 3, 200
    m = random_model(vf, K, D, seed=2)
    x = rs.randn(N, D)
    gamma = G.loglik(x, *G.tables(m.w, m.mu, m.var))[2]
    n, f, s = G.stats(x, gamma)
    n[1], f[1], s[1] = 2.5, f[1] * 2.5 / n[1], s[1] * 2.5 / n[1]                        # starved: n < D + 1
    f[2], s[2] = n[2] * 0.5, n[2] * 0.25 + 1e-9                                      # variance under the floor
    n[3], f[3], s[3] = 1e-9, 0.0, 0.0                                                # weight under the floor (and starved)
    gvar = G.global_variance(x)
    got = vf.m_step(m, G.pack_stats(n, f, s, -1.0), N, gvar)
    w, mu, var = G.m_step(n, f, s, N, m.mu, m.var, gvar)
    assert np.array_equal(got.w, w) and np.array_equal(got.mu, mu) and np.array_equal(got.var, var)
    assert np.array_equal(got.mu[1], m.mu[1]) and np.array_equal(got.var[1], m.var[1])
    assert np.array_equal(got.var[2], 0.01 * gvar)
    assert got.w[3] == 1e-6 / np.maximum(n / N, 1e-6).sum() and abs(got.w.sum() - 1.0) <= 1e-15


def test_map_adapt_agrees_with_the_reference(vf):
    m = random_model(vf, seed=3)
    x = np.random.RandomState(3).randn(150, m.D)
    gamma = G.loglik(x, *m.tables())[2]
    n, f, s = G.stats(x, gamma)
    for r in (0.0, 16.0, np.inf):
        got = vf.map_adapt(m, G.pack_stats(n, f, s, 0.0), len(x), r)
        w, mu, var = G.map_adapt(m.w, m.mu, m.var, n, f, len(x), r)
        assert np.array_equal(got.w, w) and np.array_equal(got.mu, mu) and np.array_equal(got.var, var)
    with pytest.raises(ValueError):
        vf.unpack_stats(np.zeros(7), m.K, m.D)


def test_unvoiced_files_score_nan_and_leave_every_mean(vf):
    sums = np.array([[-10.0, -8.0, -12.0], [0.0, 0.0, 0.0], [-30.0, -33.0, -27.0]])
    sc = vf.mean_scores(sums, [5, 0, 10])
    assert np.array_equal(sc[0], sums[0] / 5) and np.all(np.isnan(sc[1])) and np.array_equal(sc[2], sums[2] / 10)
    llr = sc[:, 1:] - sc[:, :1]
    d = vf.decide(llr[:, 0], llr[:, 1])
    assert d == dict(hits=1, scored=2, unvoiced=[1], flags=[True, None, False])
    assert vf.finite_mean(llr[:, 0]) == (llr[0, 0] + llr[2, 0]) / 2
    assert np.isnan(vf.finite_mean([np.nan])) and np.isnan(vf.finite_mean([]))
    assert vf.decide([], []) == dict(hits=0, scored=0, unvoiced=[], flags=[])


def test_cli_parsing(vf, tmp_path):
    a = vf._parse(["train", str(tmp_path), "-o", "ubm.npz"])
    assert (a.cmd, a.components, a.iters, a.max_utts_per_speaker, a.seed) == ("train", 64, 10, 40, 0)
    a = vf._parse(["train", str(tmp_path), "-o", "u.npz", "--components", "4", "--iters", "5", "--seed", "7",
                   "--max-utts-per-speaker", "3"])
    assert (a.components, a.iters, a.seed, a.max_utts_per_speaker, str(a.out)) == (4, 5, 7, 3, "u.npz")
    s = vf._parse(["score", "conv", "--ubm", "u.npz", "--target", "t", "--source", "s"])
    assert (s.cmd, s.enroll_utts, s.relevance, s.json) == ("score", 20, 16.0, None)
    for bad in (["train", str(tmp_path)], ["train", str(tmp_path), "-o", "u", "--components", "257"],
                ["train", str(tmp_path), "-o", "u", "--iters", "0"], ["score", "conv", "--ubm", "u.npz", "--target", "t"],
                ["score", "c", "--ubm", "u", "--target", "t", "--source", "s", "--enroll-utts", "0"], []):
        with pytest.raises(SystemExit):
            vf._parse(bad)


def test_file_lists(vf, tmp_path):
    for spk, names in (("p2", ["b.wav", "a.wav", "sub/c.wav"]), ("p1", ["z.wav"]), ("empty", [])):
        for n in names:
            (tmp_path / spk / n).parent.mkdir(parents=True, exist_ok=True)
            (tmp_path / spk / n).write_bytes(b"")
        (tmp_path / spk).mkdir(exist_ok=True)
    c = vf.corpus_files(tmp_path, 2)
    assert list(c) == ["p1", "p2"] and [f.name for f in c["p2"]] == ["a.wav", "b.wav"]
    e, r = vf.split_enrolment([tmp_path / "p2" / "b.wav", tmp_path / "p2" / "a.wav"], 1)
    assert [f.name for f in e] == ["a.wav"] and [f.name for f in r] == ["b.wav"]


def test_the_module_needs_no_gpu_to_import_and_refuses_the_cpu(vf):
    import torch
    m = random_model(vf, K=2, D=23)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vf.Verifier(m, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vf.estep(torch.zeros(4, 24), m)


def test_header_limits_are_the_modules(vf):
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    assert int(re.search(r"#define DVAE_GMM_MAX_K\s+(\d+)", hdr).group(1)) == vf.MAX_K == 256
    assert int(re.search(r"#define DVAE_GMM_MAX_DIM\s+(\d+)", hdr).group(1)) == vf.MAX_DIM == 32
    from dvae_amd import _lib
    assert {"dvae_gmm_ws_bytes", "dvae_gmm_estep", "dvae_gmm_score"} <= set(_lib.SIGNATURES)
    h = _lib.lib()
    assert h.dvae_gmm_ws_bytes(1000, 64, 23) == 4 * (64 * 47 + 1) * 8          # four tiles of 256 frames, one slot each
    assert h.dvae_gmm_ws_bytes(0, 64, 23) == 0 and h.dvae_gmm_ws_bytes(10, 257, 23) == 0
    assert h.dvae_gmm_ws_bytes(10, 1, 33) == 0
