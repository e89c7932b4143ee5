"""dvae_amd.latent_map on the MI355X: the planted speakers and the independent block through
LatentMap.map, against the float64 restatement of tests/tsne_ref.py, and the command line end to end.

The descent is chaotic at round-off level (a 1e-6 relative perturbation of the start moves final coordinates by a quarter
of the map's extent in float64), so trajectories are not compared: the GPU's final KL is held to the float64 restatement's
own spread over the same start and three perturbed ones, the printed KL to float64 on the downloaded map and tables, and the
1-NN agreements to what the restatement gives.  That inequality is a sanity check only (the gains absorb a factor-2 slip of
the gradient); tests/test_hip_tsne.py is the real check of the kernels.

Measured on the MI355X: planted speakers 1.0 / 1.0, KL 0.2455 from 2.0476 (float64 on the downloaded map 0.245458, bound
1.1e-4; the restatement from the four starts 0.2417, 0.2524, 0.2462, 0.2444); the independent block 0.207 / 0.152.
"""
import json
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import F32, F64, make_trainer
import dvae_amd  # noqa: E402,F401
import tsne_ref as R  # noqa: E402

KW = dict(perplexity=30.0, iters=400, exaggeration_iters=100)


def gpu_map(p, **kw):
    from dvae_amd import latent_map
    return latent_map.LatentMap("cuda").map(p["x"], p["speakers"], p["groups"], **dict(KW, **kw))


def kl_on(res):
    """the float64 KL on the downloaded map and affinity tables, and its bound"""
    a = {k: res["_aff"][k].astype(F64) for k in ("beta", "d2min", "lnz")}
    x, y = res["_x"], res["y"]
    d2 = R.dist2(x)
    ref = R.row_sums(R.dense_P(d2, a["beta"], a["d2min"], a["lnz"]), y)
    fb = R.forces_bound(d2, x.shape[1], a["beta"], a["d2min"], a["lnz"], y)
    Z = ref[:, 4].sum()
    bound = fb[:, 5].sum() + fb[:, 6].sum() + abs(math.log(Z)) * fb[:, 7].sum() \
        + fb[:, 4].sum() / (Z - fb[:, 4].sum()) * (ref[:, 7].sum() + fb[:, 7].sum())
    return R.kl_of(ref), bound


def test_planted_speakers_fall_into_islands():
    p = R.planted_speakers(0)
    N = len(p["x"])
    res = gpu_map(p)
    a = res["nn_agreement"]
    print(f"kl {res['kl']} from {res['kl_trace'][0][1]}, agreement {a}")
    assert a == dict(latent=1.0, map=1.0, chance=0.25)
    assert res["unconverged"] == 0 and res["non_finite_rows"] == [] and res["n_points"] == N
    assert res["rows_without_neighbour"] == dict(latent=0, map=0) and res["lr"] == 50.0
    assert [it for it, _ in res["kl_trace"]] == list(range(0, 400, 50))
    want, bound = kl_on(res)
    print(f"float64 KL on the downloaded map {want}, bound {bound:.3g}")
    assert bound < 1e-3 and abs(res["kl"] - want) <= bound
    # the float64 restatement from the same start and three perturbed ones: its own spread is the margin
    d2 = R.dist2(p["x"])
    af = R.affinities(d2, 30.0)
    P = R.dense_P(d2, af["beta"], af["d2min"], af["lnz"])
    y0 = R.pca_init(p["x"])
    rs = np.random.RandomState(0)
    kls = [R.embed(P, y0 * (1.0 + 1e-6 * s * rs.randn(*y0.shape)), 400, 100, 12.0, 50.0)["kl"] for s in (0, 1, 1, 1)]
    print(f"float64 restatement: {kls}")
    assert res["kl_trace"][0][1] > 1.5 and res["kl"] <= max(kls) + (max(kls) - min(kls))
    # the same map twice
    again = gpu_map(p)
    assert np.array_equal(again["y"].view(np.uint32), res["y"].view(np.uint32)) and again["kl"] == res["kl"]
    # a random start is another map, the same islands
    rnd = gpu_map(p, init="random", seed=3)
    assert rnd["nn_agreement"]["map"] == 1.0 and not np.array_equal(rnd["y"], res["y"])


def test_an_independent_block_stays_at_chance():
    res = gpu_map(R.planted_independent(0))
    a = res["nn_agreement"]
    print(f"agreement {a}")
    assert a["chance"] == 0.25 and a["latent"] < 0.40 and a["map"] < 0.40
    assert res["unconverged"] == 0


def test_too_few_points_for_the_perplexity():
    p = R.planted_speakers(0, per=16)
    with pytest.raises(ValueError, match=r"perplexity 30.*64 points"):
        gpu_map(p)
    with pytest.raises(ValueError, match="pca or random"):
        gpu_map(p, perplexity=5.0, init="zeros")


def test_a_non_finite_row_is_listed_and_left_out():
    p = R.planted_speakers(1, per=16)
    x = p["x"].copy()
    x[5, 1] = np.nan
    x[40, 0] = np.inf
    keep = np.ones(64, bool)
    keep[[5, 40]] = False
    kw = dict(perplexity=5.0, iters=60, exaggeration_iters=20)
    res = gpu_map(dict(p, x=x), **kw)
    clean = gpu_map({k: v[keep] for k, v in p.items()}, **kw)
    assert res["non_finite_rows"] == [5, 40] and res["n_points"] == 62 and res["kept"].tolist() == np.flatnonzero(keep).tolist()
    assert np.array_equal(res["y"].view(np.uint32), clean["y"].view(np.uint32)) and res["kl"] == clean["kl"]
    assert res["nn_agreement"] == clean["nn_agreement"]


def test_the_pieces_agree_with_the_restatement():
    """nearest, affinities and one embed step through the Python layer"""
    from dvae_amd import latent_map
    p = R.planted_speakers(2, per=16)
    lm = latent_map.LatentMap("cuda")
    d2 = R.dist2(p["x"])
    for grp in (None, p["groups"]):
        _, arg = lm.nearest(p["x"], grp)
        assert np.array_equal(arg.cpu().numpy(), R.nearest(d2, grp)[1])
    aff = lm.affinities(p["x"], 5.0)
    b, dm = aff["beta"].cpu().numpy().astype(F64), aff["d2min"].cpu().numpy().astype(F64)
    _, h64 = R.entropy_at(d2, dm, b)
    _, bh = R.affinities_bound(d2, 4, dm, b)
    assert np.all(np.abs(h64 - math.log(5.0)) <= 1.01e-5 + bh) and np.all(aff["steps"].cpu().numpy() >= 1)
    y0 = R.pca_init(p["x"]).astype(F32)
    e = lm.embed(p["x"], aff, y0, 1, 1, 12.0, 50.0, kl_every=1)
    affh = {k: v.cpu().numpy() for k, v in aff.items()}
    want, bound = kl_on(dict(_aff=affh, _x=p["x"], y=y0))
    assert e["kl_trace"][0][0] == 0 and abs(e["kl_trace"][0][1] - want) <= bound      # the KL before the first update
    want, bound = kl_on(dict(_aff=affh, _x=p["x"], y=e["y"].cpu().numpy()))
    assert abs(e["kl"] - want) <= bound and not np.array_equal(e["y"].cpu().numpy(), y0)


# --------------------------------------------------------------------------------------------------------- end to end
def test_cli_end_to_end(tmp_path, capsys):
    from dvae_amd import latent_map
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=3, n_utt=4, length=130)
    run_dir = tmp_path / "run"
    (run_dir / "checkpoints").mkdir(parents=True)
    cfg = dict(samples_length=64, latent_size=32, speaker_size=4, lr=1e-4, batch_size=4, mse_cof=10, kl_cof=10)
    (run_dir / "config.json").write_text(json.dumps(cfg))
    w = make_trainer(batch=4, n_frames=64)
    torch.save(w.model.state_dict(), run_dir / "checkpoints" / "DisentangledVAE_VCTK_2.pth")
    argv = [corpus, "--log_dir", str(run_dir), "--seed", "3", "--perplexity", "5", "--iters", "120"]
    assert latent_map.main(argv) == 0
    out = capsys.readouterr().out.splitlines()
    files = ["latent_map.json"] + [f"latent_map_{b}.{e}" for b in ("style", "content", "joint") for e in ("npy", "svg")]
    first = {f: (run_dir / f).read_bytes() for f in files}
    res = json.loads(first["latent_map.json"])
    assert res["lines"] == out[:3] and res["checkpoint_epoch"] == 2 and res["level"] == "chunk"
    num = r"(-?[0-9.e+-]+|nan|inf)"
    for k, b in enumerate(("style", "content", "joint")):
        m = re.match(rf"^latent map {b}: (\d+) points, perplexity {num}, kl {num} \(from {num}\), 1-nn speaker agreement: "
                     rf"latent {num}, map {num} \(chance {num}\), unconverged rows (\d+)$", out[k])
        assert m, out[k]
        r = res["blocks"][b]
        assert int(m.group(1)) == r["n_points"] == 24 and int(m.group(8)) == r["unconverged"]
        assert [float(m.group(i)) for i in (2, 3, 4, 5, 6, 7)] == [5.0, r["kl"], r["kl_trace"][0][1], r["nn_agreement"]["latent"],
                                                                  r["nn_agreement"]["map"], r["nn_agreement"]["chance"]]
        assert abs(r["nn_agreement"]["chance"] - 1.0 / 3.0) <= 1e-12 and math.isfinite(r["kl"])
        y = np.load(run_dir / f"latent_map_{b}.npy")
        assert y.shape == (24, 2) and y.dtype == np.float32 and np.isfinite(y).all()
        svg = first[f"latent_map_{b}.svg"].decode()
        assert svg.count("<circle ") == 24 and all(s in svg for s in ("spk000", "spk001", "spk002"))
    # a second run is byte-identical in all of them
    assert latent_map.main(argv) == 0
    capsys.readouterr()
    for f in files:
        assert (run_dir / f).read_bytes() == first[f], f
    # utterances as the points, one block, no picture
    assert latent_map.main(argv[:3] + ["--level", "utterance", "--block", "style", "--perplexity", "3", "--iters", "30", "--no-svg",
                                       "--json", str(tmp_path / "u.json")]) == 0
    u = json.loads((tmp_path / "u.json").read_text())
    assert list(u["blocks"]) == ["style"] and u["blocks"]["style"]["n_points"] == 12
    assert (run_dir / "latent_map_style.svg").read_bytes() == first["latent_map_style.svg"]      # not rewritten
    # too few points for the default perplexity: an argument error
    assert latent_map.main(argv[:3]) == 2
    assert "perplexity" in capsys.readouterr().err
