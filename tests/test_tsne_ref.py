"""The float64 restatement of the latent map (tests/tsne_ref.py) on the CPU: against scikit-learn's
exact t-SNE where it is installed, the matrix-free row sums against the dense gradient, fp32 walks in the kernels' order
inside the derived bounds on every shape of tests/test_hip_tsne.py, and the plumbing (header, binding, constants, the SVG
writer, command-line errors).

Measured here: P against scikit-learn's _joint_probabilities 2.8e-8 max P (planted speakers, N = 256, D = 4, perplexity 30);
KL and gradient against _kl_divergence 4e-15 and 2e-15 relative; worst error / bound of the fp32 walks over the GPU shapes:
distance 0.998 (D = 1: three roundings, all of them met), lnz 0.255, entropy 0.096, forces 0.354, update 0.976.
"""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tsne_ref as R  # noqa: E402
from ref_common import EPS32, F, F64, fma, worst_ratio  # noqa: E402


@pytest.fixture(scope="module")
def planted():
    p = R.planted_speakers(0)
    d2 = R.dist2(p["x"])
    a = R.affinities(d2, 30.0)
    return dict(p, d2=d2, aff=a, P=R.dense_P(d2, a["beta"], a["d2min"], a["lnz"]))


# ------------------------------------------------------------------------------------------------ against scikit-learn
def test_joint_probabilities_against_sklearn(planted):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    ref = squareform(_t_sne._joint_probabilities(planted["d2"], 30.0, 0))
    err = np.abs(planted["P"] - ref).max() / ref.max()
    print(f"P against scikit-learn: {err:.3g} max P")
    assert err <= 3e-5
    assert (planted["aff"]["steps"] > 0).all() and abs(planted["P"].sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("scale", [1e-4, 1.0])
def test_kl_and_gradient_against_sklearn(planted, scale):
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    N = len(planted["x"])
    y = np.random.RandomState(1).randn(N, 2) * scale
    kl, grad = _t_sne._kl_divergence(y.ravel(), squareform(planted["P"], checks=False), 1.0, N, 2)
    rows = R.row_sums(planted["P"], y)
    ek = abs(R.kl_of(rows) - kl) / abs(kl)
    eg = np.abs(R.gradient_of(rows).ravel() - grad).max() / np.abs(grad).max()
    print(f"scale {scale}: kl {ek:.3g}, gradient {eg:.3g} relative")
    assert ek <= 1e-12 and eg <= 1e-12


def test_row_sums_reproduce_the_dense_gradient_and_kl(planted):
    P, N = planted["P"], len(planted["x"])
    y = np.random.RandomState(2).randn(N, 2)
    dy = y[:, None] - y[None]
    w = 1.0 / (1.0 + (dy ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    Q = w / w.sum()
    off = ~np.eye(N, dtype=bool)
    kl = float((P[off & (P > 0)] * np.log(P[off & (P > 0)] / Q[off & (P > 0)])).sum())
    for ex in (1.0, 12.0):
        grad = 4.0 * (((ex * P - Q) * w)[..., None] * dy).sum(1)
        rows = R.row_sums(P, y)
        assert np.abs(R.gradient_of(rows, ex) - grad).max() <= 1e-12 * np.abs(grad).max()
    assert abs(R.kl_of(rows) - kl) <= 1e-12 * abs(kl)
    assert (R.row_sums(P, y, want_kl=False)[:, 5:] == 0).all()


def test_the_restatement_embeds_the_planted_speakers(planted):
    N = len(planted["x"])
    e = R.embed(planted["P"], R.pca_init(planted["x"]), 400, 100, 12.0, max(N / 12.0 / 4.0, 50.0))
    print(f"kl {e['kl']:.4f} from {e['trace'][0][1]:.4f}")
    assert e["kl"] < 0.3 < 2.0 < e["trace"][0][1]
    for X in (planted["x"], e["y"]):
        _, arg = R.nearest(R.dist2(X), planted["groups"])
        assert R.nn_agreement(arg, planted["speakers"]) == (1.0, 0)
    assert R.chance(planted["speakers"]) == 0.25


def test_nearest_admissibility_ties_and_rows_without_a_neighbour():
    x = np.array([[0.0], [1.0], [1.0], [5.0]])
    d2 = R.dist2(x)
    best, arg = R.nearest(d2)
    assert arg.tolist() == [1, 2, 1, 1] and best.tolist() == [1.0, 0.0, 0.0, 16.0]
    best, arg = R.nearest(d2, np.array([0, 0, 1, 1]))
    assert arg.tolist() == [2, 2, 1, 1]
    best, arg = R.nearest(d2, np.zeros(4, int))
    assert arg.tolist() == [-1] * 4 and np.isinf(best).all()
    assert R.nn_agreement(arg, np.zeros(4)) [1] == 4 and math.isnan(R.nn_agreement(arg, np.zeros(4))[0])
    assert R.nn_agreement(np.array([1, 0, -1]), np.array([0, 1, 1])) == (0.0, 1)


def test_more_ties_than_the_perplexity_do_not_converge():
    c = R.kernel_case(63, 4, 4)
    x = c["x"].copy()
    x[10:17] = x[10]
    a = R.affinities(R.dist2(x), 5.0)
    assert (a["steps"][10:17] == -1).all() and (np.delete(a["steps"], np.s_[10:17]) > 0).all()
    assert np.isfinite(a["beta"]).all() and np.isfinite(a["lnz"]).all() and np.isfinite(a["entropy"]).all()
    assert np.all(a["entropy"][10:17] > math.log(6.0) - 1e-9)


# -------------------------------------------------------------------------------------------------------------- bounds
_WALKS = {}


def walk(D, ld):
    """the worst error / bound per family of the fp32 walks over every N of the GPU suite at (D, ld); computed once"""
    if (D, ld) in _WALKS:
        return _WALKS[(D, ld)]
    worst = {}

    def held(key, got, ref, bound):
        r, at = worst_ratio(got, ref, bound)
        assert r <= 1.0, (key, D, at, r)
        worst[key] = max(worst.get(key, 0.0), r)

    for N in R.NS:
        c = R.kernel_case(N, D, ld)
        d2, d32 = c["d2"], R.dist2_f32(c["x"])
        held("distance", d32, d2, R.dist_bound(d2, D))
        assert np.array_equal(d32, d32.T)
        for grp in (None, c["group"]):
            a64 = R.nearest(d2, grp)[1]
            assert np.array_equal(R.nearest(d32.astype(F64), grp)[1], a64), (N, D)
        assert a64[4] == 2 and (c["aff"]["steps"] > 0).all() and c["aff"]["steps"].max() <= R.MAX_STEPS
        d2min = R.nearest(d32.astype(F64))[0].astype(F)
        beta = c["aff"]["beta"].astype(F)
        lnz, H = R.affinity_sums_f32(d32, d2min, beta)
        l64, h64 = R.entropy_at(d2, d2min.astype(F64), beta.astype(F64))
        bl, bh = R.affinities_bound(d2, D, d2min.astype(F64), beta.astype(F64))
        held("lnz", lnz, l64, bl)
        held("entropy", H, h64, bh)
        # not vacuous where it matters: an ordinary row's entropy is held to a thousandth of a nat (the worst case of a
        # distance of 64 dimensions is 4e-6 relative, times beta d; at N = 8 most rows are planted ones)
        assert N == 8 or np.median(bh) < 1e-3, (N, D, np.median(bh))
        t = R.forces_inputs(c)
        t64 = {k: v.astype(F64) for k, v in t.items()}
        rows = R.forces_f32(d32, t["beta"], t["d2min"], t["lnz"], c["y"])
        ref = R.row_sums(R.dense_P(d2, t64["beta"], t64["d2min"], t64["lnz"]), c["y"])
        fb = R.forces_bound(d2, D, t64["beta"], t64["d2min"], t64["lnz"], c["y"])
        assert np.isfinite(rows).all() and np.isfinite(fb).all() and (fb > 0).all()
        held("forces", rows, ref, fb)
        u = R.update_case(c)
        rw, y, up, gn = (np.asarray(v, F) for v in (u["rows"], c["y"], u["upd"], u["gains"]))
        izf = F(1.0 / rw[:, 4].astype(F64).sum())
        g32 = F(4) * fma(F(u["ex"]), rw[:, 0:2], -(rw[:, 2:4] * izf))
        gnew = np.maximum(np.where(up * g32 < 0, gn + F(0.2), gn * F(0.8)), F(R.MIN_GAIN))
        un = fma(F(u["momentum"]), up, -(F(u["lr"]) * (gnew * g32)))
        held("update", g32, u["ref"]["g"], u["bound"]["g"])
        held("update", un, u["ref"]["upd"], u["bound"]["upd"])
        held("update", y + un, u["ref"]["y"], u["bound"]["y"])
        assert np.array_equal(gnew, u["ref"]["gains"])
    _WALKS[(D, ld)] = worst
    return worst


@pytest.mark.parametrize("D,ld", R.SHAPES)
def test_fp32_walks_in_the_kernels_order_stay_inside_the_bounds(D, ld):
    w = walk(D, ld)
    print(f"D {D}: worst error / bound of the fp32 walks: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))


def test_the_bounds_are_not_a_hundred_times_too_wide():
    ws = [walk(D, ld) for D, ld in R.SHAPES]
    worst = {k: max(w[k] for w in ws) for k in ws[0]}
    print("worst error / bound of the fp32 walks: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert min(worst.values()) > 0.05, worst


# ------------------------------------------------------------------------------------------------------------ plumbing
def test_header_and_binding_agree():
    from dvae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    assert int(re.search(r"#define DVAE_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 319
    assert int(re.search(r"#define DVAE_LATENT_MAX_D (\d+)", hdr).group(1)) == R.MAX_D
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("dvae_tsne_nn", "dvae_tsne_affinities", "dvae_tsne_forces", "dvae_tsne_update"):
        m = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    csrc = os.path.join(ROOT, "disentangle-vae-for-vc_amd", "csrc")
    src = open(os.path.join(csrc, "tsne.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")
    probe = open(os.path.join(csrc, "probe.hip")).read()
    assert probe.index('#include "latents.hip"') < probe.index('#include "tsne.hip"')
    assert "tsne.hip" in open(os.path.join(csrc, "build.sh")).read()


def test_module_constants_follow_the_reference():
    from dvae_amd import latent_map as M
    assert (M.MAX_D, M.MAX_STEPS, M.ENTROPY_TOL) == (R.MAX_D, R.MAX_STEPS, R.ENTROPY_TOL)
    src = open(os.path.join(ROOT, "disentangle-vae-for-vc_amd", "csrc", "tsne.hip")).read()
    assert "TS_ENTROPY_TOL = 1e-5f" in src and "TS_BETA_MAX = 0x1p100f" in src and "TS_MIN_GAIN = 0.01f" in src
    p = R.planted_speakers(1, per=16)
    assert np.array_equal(M.pca_init(p["x"]), R.pca_init(p["x"]))
    assert np.array_equal(M.pca_init(p["x"][:, :1], 3), R.pca_init(p["x"][:, :1], 3))
    y0 = M.pca_init(p["x"])
    assert abs(y0[:, 0].std() - 1e-4) <= 1e-16 and abs(y0.mean(0)).max() <= 1e-16
    arg = np.array([1, 0, -1, 2])
    spk = np.array([0, 0, 1, 1])
    assert M.nn_agreement(arg, spk) == R.nn_agreement(arg, spk) == (1.0, 1)
    assert M.chance(np.array([0, 0, 0, 1])) == R.chance(np.array([0, 0, 0, 1])) == 0.625
    rows = np.random.RandomState(0).rand(50, 8)
    assert abs(M.kl_of_rows(rows) - R.kl_of(rows)) <= 1e-12
    m, ids = M.utterance_means(np.array([[1.0], [3.0], [5.0]]), np.array([7, 7, 9]))
    assert m.tolist() == [[2.0], [5.0]] and ids.tolist() == [7, 9]


def test_svg_is_byte_stable_and_escapes_names():
    from dvae_amd import latent_map as M
    rs = np.random.RandomState(0)
    y, spk = rs.randn(37, 2), rs.randint(0, 3, 37)
    names = ["a<b", "c&d", 'e"f']
    s1, s2 = M.svg_scatter(y, spk, names, title="t <1>"), M.svg_scatter(y.copy(), spk.copy(), list(names), title="t <1>")
    assert s1 == s2 and s1.count("<circle ") == 37
    assert "a&lt;b" in s1 and "c&amp;d" in s1 and "a<b" not in s1 and "t &lt;1&gt;" in s1
    assert s1.startswith("<svg ") and s1.endswith("</svg>\n")
    import xml.dom.minidom
    xml.dom.minidom.parseString(s1)
    for k in range(3):
        assert s1.count(f'fill="{M.PALETTE[k]}"') == int((spk == k).sum()) + 1      # its circles and its legend entry
    # a single point and coincident points do not divide by zero
    assert M.svg_scatter(np.zeros((2, 2)), [0, 1], ["x", "y"]).count("<circle ") == 2


def test_cli_argument_errors(tmp_path, capsys):
    from dvae_amd import latent_map as M
    t = str(tmp_path)
    assert M.main([]) == 2
    assert M.main([t]) == 2                                                    # no --log_dir
    assert M.main([t, "--log_dir", t, "--no-such-flag"]) == 2
    assert M.main([t, "--log_dir", t, "--block", "other"]) == 2
    assert M.main([t, "--log_dir", t, "--level", "frame"]) == 2
    assert M.main([t, "--log_dir", t, "--init", "zeros"]) == 2
    assert M.main([t, "--log_dir", t]) == 2                                    # no config.json
    (tmp_path / "config.json").write_text("{}")
    assert M.main([str(tmp_path / "nowhere"), "--log_dir", t]) == 2
    assert M.main([t, "--log_dir", t, "--max-chunks", "0"]) == 2
    assert M.main([t, "--log_dir", t, "--perplexity", "0.5"]) == 2
    assert M.main([t, "--log_dir", t, "--iters", "0"]) == 2
    assert M.main([t, "--log_dir", t]) == 1                                    # no checkpoint: not an argument error
    assert "latent_map:" in capsys.readouterr().err
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.LatentMap("cpu")
