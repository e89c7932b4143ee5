"""CPU checks of the i-vector speaker embeddings: the float64 restatement tests/ivector_ref.py holds
what the GPU suite builds on (the explicit Cholesky walk stays inside every bound against numpy.linalg on every GPU shape,
EM ascends with and without the minimum-divergence step, the planted speakers are separable by a margin no rounding turns,
the equal error rate agrees with a brute-force sweep and with scikit-learn), and dvae_amd.ivector's host logic, bindings,
command line and file format agree with it."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_ref as G  # noqa: E402
import ivector_ref as I  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted_stats(p, rows=None):
    """float64 statistics of the planted utterances under the UBM's fp32 tables -> n, f, (a, mu, prec), gamma"""
    tab = G.tables(*p["ubm"])
    gamma = G.loglik(p["x"], *tab)[2]
    n, g, _, _ = I.utt_sums(p["x"], gamma, p["segs"])
    return n, I.centre_whiten(n, g, tab[1], tab[2]), tab, gamma


def split(p, held=2):
    """training utterances: all but the last `held` of every speaker"""
    idx = np.arange(len(p["speaker"])) % p["utts"]
    return idx < p["utts"] - held


# ------------------------------------------------------------------------------------------ the walk inside the bounds
@pytest.mark.parametrize("U,K,D,R", I.POSTERIOR_SHAPES)
def test_walk_against_linalg_inside_every_bound(U, K, D, R):
    n, f, T = I.posterior_inputs(U, K, D, R)
    P = I.gram(T, K, D)
    p, q = I.posterior(n, f, T, P), I.posterior_linalg(n, f, T, P)
    worst = dict(back_w=0.0, back_inv=0.0, fwd_w=0.0, fwd_ll=0.0, fwd_S=0.0, kappa=0.0)
    for u in range(U):
        rw, ri = I.backward_ratios(p["L"][u], p["b"][u], p["w"][u], p["S"][u], K, D, R)
        bw, bll, kappa = I.forward_bounds(q["L"][u], q["w"][u], q["ll"][u], K, D, R)
        assert kappa * I.eps_b(K, D, R) < 0.25, "the forward form needs kappa eps_b well below 1"
        worst["back_w"], worst["back_inv"] = max(worst["back_w"], rw), max(worst["back_inv"], ri)
        worst["fwd_w"] = max(worst["fwd_w"], np.linalg.norm(p["w"][u] - q["w"][u]) / bw)
        worst["fwd_ll"] = max(worst["fwd_ll"], abs(p["ll"][u] - q["ll"][u]) / bll)
        worst["fwd_S"] = max(worst["fwd_S"], np.linalg.norm(p["S"][u] - q["S"][u]) /
                             I.s_forward_bound(q["L"][u], q["w"][u], q["inv"][u], K, D, R))
        worst["kappa"] = max(worst["kappa"], kappa)
    print(f"\n(U, K, D, R) = {(U, K, D, R)}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for k, v in worst.items() if k != "kappa"), worst
    if U >= 3:
        assert worst["kappa"] > 1e5, "the scaled utterance is ill-conditioned"
    if U >= 2:                                               # the all-zero utterance: exact
        assert np.array_equal(p["w"][-1], np.zeros(R)) and np.array_equal(p["S"][-1], np.eye(R)) and p["ll"][-1] == 0.0


def test_nonfinite_input_stays_in_its_utterance():
    n, f, T = I.posterior_inputs(7, 4, 5, 3)
    f[2, 1] = np.nan
    p = I.posterior(n, f, T, I.gram(T, 4, 5))
    bad = ~np.isfinite(p["w"]).all(axis=1)
    assert bad.tolist() == [u == 2 for u in range(7)]


# ------------------------------------------------------------------------------------------------------------------- EM
@pytest.mark.parametrize("min_div", [True, False])
def test_em_ascends(min_div):
    p = I.planted()
    n, f, _, _ = planted_stats(p)
    _, lls = I.em(n, f, p["K"], p["D"], p["R"], 8, min_div=min_div, post=I.posterior)
    assert len(lls) == 8 and np.all(np.isfinite(lls))
    assert np.min(np.diff(lls)) >= -1e-12 * (1.0 + np.max(np.abs(lls))), np.diff(lls)
    assert lls[-1] > lls[0] + 1.0, "EM moved"


def test_starved_component_keeps_its_rows():
    p = I.planted()
    n, f, _, _ = planted_stats(p)
    n2 = n.copy()
    n2[:, 1] = 1e-6 / len(n)
    T = I.init_T(p["K"], p["D"], p["R"], 0)
    T2, _, _ = I.em_step(n2, f, T, p["K"], p["D"], min_div=False)
    D = p["D"]
    assert np.array_equal(T2[D:2 * D], T[D:2 * D]) and not np.array_equal(T2[:D], T[:D])


def test_planted_speakers_are_separable_by_a_margin_no_rounding_turns():
    p = I.planted()
    K, D, R = p["K"], p["D"], p["R"]
    n, f, tab, gamma = planted_stats(p)
    tr, spk = split(p), p["speaker"]
    assert tr.sum() == 36 and len(p["x"]) == 6 * 8 * 60
    T, _ = I.em(n[tr], f[tr], K, D, R, 8)
    P = I.gram(T, K, D)
    post = I.posterior(n, f, T, P)
    cos, mean, W = I.identify(post["w"][tr], spk[tr], post["w"][~tr])
    gap = I.margin(cos, spk[~tr])
    # what an fp32 gamma inside its bound, float64 sums and the posterior's forward error can move an i-vector by
    q = G.loglik(p["x"], *tab)[3]
    gb = G.gamma_bound(tab[0], gamma, q, D)
    dw = 0.0
    for u, (r0, c) in enumerate(p["segs"]):
        dn, df = I.gamma_input_bounds(gb[r0:r0 + c], p["x"][r0:r0 + c], tab[1], tab[2])
        dw = max(dw, I.w_input_bound(dn, df, T, P, post["L"][u], post["w"][u]) +
                 I.forward_bounds(post["L"][u], post["w"][u], post["ll"][u], K, D, R)[0])
    bound = I.cosine_bound(dw, post["w"], mean, W)
    print(f"\nplanted speakers: smallest cosine margin {gap:.4f}, propagated bound {bound:.3g}")
    assert gap > 0, "the float64 pipeline itself misses an utterance"
    assert gap > 100 * bound, (gap, bound)                   # two orders above a bound that is itself a worst case
    assert np.array_equal(np.argmax(cos, axis=1), spk[~tr])


# ------------------------------------------------------------------------------------------------------------------ EER
def roc_eer(tar, non):
    from sklearn.metrics import roc_curve
    y = np.concatenate([np.ones(len(tar)), np.zeros(len(non))])
    fpr, tpr, thr = roc_curve(y, np.concatenate([tar, non]), drop_intermediate=False)
    # roc_curve walks the thresholds downwards from "accept nothing"; ours go upwards
    return I.cross(fpr[::-1], 1.0 - tpr[::-1], np.where(np.isfinite(thr[::-1]), thr[::-1], np.max(thr[np.isfinite(thr)])))[0]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_eer_against_brute_force_and_sklearn(seed):
    from dvae_amd import ivector
    rs = np.random.RandomState(seed)
    tar, non = rs.randn(37) + 1.0 + 0.5 * seed, rs.randn(211)
    if seed % 2:                                             # ties inside and across the two lists
        tar, non = np.round(tar * 4) / 4, np.round(non * 4) / 4
    e, t = ivector.eer(tar, non)
    assert (e, t) == I.eer(tar, non) == I.eer_brute(tar, non)
    assert abs(e - roc_eer(tar, non)) <= 1e-12
    assert 0.0 < e < 0.5 and tar.min() <= t <= non.max()


def test_eer_edges():
    from dvae_amd import ivector
    assert ivector.eer([2.0, 3.0], [0.0, 1.0]) == (0.0, 2.0) == I.eer_brute([2.0, 3.0], [0.0, 1.0])
    assert ivector.eer([0.0, 1.0], [2.0, 3.0]) == (1.0, 2.0) == I.eer_brute([0.0, 1.0], [2.0, 3.0])
    assert ivector.eer([1.0, 1.0], [1.0, 1.0])[0] == 0.5      # one tie of everything: the crossing between the two points
    assert abs(roc_eer(np.array([2.0, 3.0]), np.array([0.0, 1.0]))) == 0.0
    assert roc_eer(np.array([0.0, 1.0]), np.array([2.0, 3.0])) == 1.0
    for bad in (([np.nan, 1.0], [0.0]), ([1.0], [np.nan]), ([], [1.0]), ([1.0], [])):
        with pytest.raises(ValueError):
            ivector.eer(*bad)


# ------------------------------------------------------------------------------------------------------- the host logic
def test_host_functions_agree_with_the_restatement():
    from dvae_amd import ivector
    p = I.planted()
    K, D, R = p["K"], p["D"], p["R"]
    n, f, _, _ = planted_stats(p)
    T = I.init_T(K, D, R, 3)
    assert np.array_equal(ivector.initial_T(K, D, R, 3), T) and ivector.INIT_SCALE == I.INIT_SCALE
    assert np.array_equal(ivector.gram(T, D), I.gram(T, K, D))
    post = I.posterior(n, f, T, I.gram(T, K, D))
    A, C, Ssum = I.accumulators(n, f, post["w"], post["S"])
    T2 = ivector.m_step(T, A, C, n.sum(axis=0), D)
    assert np.array_equal(T2, I.m_step(T, A, C, n.sum(axis=0), K, D)) and ivector.N_FLOOR == I.N_FLOOR
    assert np.array_equal(ivector.apply_min_divergence(T2, Ssum, len(n)), I.min_divergence(T2, Ssum, len(n)))
    w = post["w"].copy()
    be = ivector.Backend.fit(w)
    mean, W = I.backend_fit(w)
    assert np.array_equal(be.mean, mean) and np.array_equal(be.W, W)
    y = be.transform(w)
    assert np.array_equal(y, I.backend_transform(w, mean, W)) and np.allclose(np.linalg.norm(y, axis=1), 1.0, atol=1e-15)
    yc = (w - mean) @ W
    assert np.allclose(yc.T @ yc / len(w), np.eye(R), atol=1e-10), "the training i-vectors come out white"
    w[5] = np.nan
    y = be.transform(w)
    assert np.isnan(y[5]).all() and np.isfinite(np.delete(y, 5, axis=0)).all()
    assert np.array_equal(ivector.Backend.speaker(y[:8]), I.speaker_model(np.delete(y[:8], 5, axis=0)))
    cos = ivector.cosine_scores(y, y[:2])
    assert np.isnan(cos[5]).all() and np.allclose(np.delete(cos, 5, axis=0), I.cosine(np.delete(y, 5, axis=0), y[:2]))
    with pytest.raises(ValueError):
        ivector.Backend.speaker(y[5:6])


def test_bindings_mirror_the_header():
    from dvae_amd import _lib, ivector
    text = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    assert int(re.search(r"#define DVAE_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 319
    assert int(re.search(r"#define DVAE_IVEC_MAX_R (\d+)", text).group(1)) == ivector.MAX_R == 64
    assert ivector.SYMBOLS == ("dvae_gmm_utt_stats", "dvae_ivec_posterior", "dvae_ivec_ws_bytes", "dvae_ivec_accumulate")
    for name in ivector.SYMBOLS:
        m = re.search(r"^(\w+) " + name + r"\(([^;]*)\);", text, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/dvae_hip.h"
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(m.group(2).split(",")), name
        assert (res is _lib.C.c_size_t) == (m.group(1) == "size_t")
        for a, decl in zip(args, m.group(2).split(",")):
            assert (a is _lib.vp) == ("*" in decl), (name, decl)


def test_a_library_without_the_symbols_asks_for_a_rebuild(monkeypatch):
    from dvae_amd import ivector
    monkeypatch.setattr(ivector, "lib", lambda: object())
    with pytest.raises(RuntimeError, match="rebuild the library"):
        ivector._lib()


@pytest.mark.parametrize("argv", [
    [], ["train"], ["train", "root", "-o", "x.npz"], ["train", "root", "--ubm", "u.npz"],
    ["train", "root", "--ubm", "u.npz", "-o", "x.npz", "--rank", "0"],
    ["train", "root", "--ubm", "u.npz", "-o", "x.npz", "--rank", "65"],
    ["train", "root", "--ubm", "u.npz", "-o", "x.npz", "--iters", "0"],
    ["train", "root", "--ubm", "u.npz", "-o", "x.npz", "--max-utts-per-speaker", "0"],
    ["score", "conv", "--ubm", "u.npz", "--ivector", "i.npz", "--target", "t"],
    ["score", "conv", "--ubm", "u.npz", "--target", "t", "--source", "s"],
    ["score", "conv", "--ubm", "u.npz", "--ivector", "i.npz", "--target", "t", "--source", "s", "--enroll-utts", "0"],
    ["eer", "root", "--ubm", "u.npz"], ["eer", "root", "--ubm", "u.npz", "--ivector", "i.npz", "--enroll-utts", "0"],
    ["eer", "root", "--ubm", "u.npz", "--ivector", "i.npz", "--enroll-utts", "5", "--max-utts-per-speaker", "5"],
    ["convert", "x"]])
def test_cli_refuses_bad_arguments(argv, capsys):
    from dvae_amd import ivector
    with pytest.raises(SystemExit) as e:
        ivector.main(argv)
    assert e.value.code == 2
    capsys.readouterr()


def test_cli_missing_directories_exit_2(tmp_path, capsys):
    from dvae_amd import ivector, verify
    ubm = tmp_path / "ubm.npz"
    verify.DiagGMM(np.ones(2) / 2, np.zeros((2, 23)), np.ones((2, 23))).save(ubm)
    missing = str(tmp_path / "nowhere")
    assert ivector.main(["train", missing, "--ubm", str(ubm), "-o", str(tmp_path / "i.npz")]) == 2
    assert ivector.main(["score", missing, "--ubm", str(ubm), "--ivector", "i.npz", "--target", missing, "--source",
                         missing]) == 2
    assert ivector.main(["eer", missing, "--ubm", str(ubm), "--ivector", "i.npz"]) == 2
    assert "is not a directory" in capsys.readouterr().err


def test_save_load_round_trip_and_the_ubm_mismatch(tmp_path):
    from dvae_amd import ivector, verify
    rs = np.random.RandomState(0)
    K, D, R = 3, 23, 4
    ubm = verify.DiagGMM(np.ones(K) / K, rs.randn(K, D), rs.uniform(0.5, 2.0, (K, D)))
    T = rs.randn(K * D, R)
    be = ivector.Backend(rs.randn(R), rs.randn(R, R))
    config = dict(rank=R, iters=7, seed=5, min_divergence=False, batch=4096, n_floor=ivector.N_FLOOR,
                  init_scale=ivector.INIT_SCALE, eig_floor=ivector.EIG_FLOOR, utterances=12)
    ex = ivector.Extractor(ubm, T, be, "cuda", config)
    path = tmp_path / "ivec.npz"
    ex.save(path)
    for given in (None, ubm):
        back = ivector.Extractor.load(path, given)
        assert np.array_equal(back.T, T) and np.array_equal(back.backend.mean, be.mean) and np.array_equal(back.backend.W, be.W)
        assert np.array_equal(back.ubm.w, ubm.w) and np.array_equal(back.ubm.mu, ubm.mu) and np.array_equal(back.ubm.var, ubm.var)
        assert back.config == config and back.config["batch"] == 4096 and back.rank == R
    with np.load(path) as z:
        for k, v in verify.FEATURE_CONSTANTS.items():
            assert z[k].item() == v
    other = verify.DiagGMM(ubm.w, ubm.mu + 1e-9, ubm.var)
    with pytest.raises(ValueError, match="another UBM"):
        ivector.Extractor.load(path, other)
    with pytest.raises(ValueError, match="another UBM"):
        ivector.Extractor.load(path, verify.DiagGMM(np.ones(2) / 2, np.zeros((2, D)), np.ones((2, D))))
    with pytest.raises(ValueError):
        ivector.Extractor(ubm, T[:-1], be)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ivector.Extractor(ubm, T, be, "cpu")
    ivector.Extractor(ubm, T).save(tmp_path / "nobackend.npz")
    assert ivector.Extractor.load(tmp_path / "nobackend.npz").backend is None
