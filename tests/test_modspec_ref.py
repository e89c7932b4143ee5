"""Over-smoothing instruments (dvae_amd.modspec), the CPU half: the properties of the float64 restatement in
tests/modspec_ref.py (Parseval, the identities of the postfilter, the offset and the clamp, restoration of a known
attenuation), the statistics container, the host plan, the argument checks of the two commands and the ABI number."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
import modspec_ref as M  # noqa: E402
from dvae_amd import convert, modspec  # noqa: E402

F32, F64 = np.float32, np.float64


def _windows(seed, n=12, C=3, D=16):
    return M.trajectories(np.random.RandomState(seed), (n, C, D))


# ------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("D", [8, 10, 64, 128])
def test_parseval(D):
    w = _windows(D, 5, 3, D)
    _, d, Y = M.analyse(w)
    var = (d * d).sum(-1) / D
    assert np.allclose(var, (M.weights(D) * np.abs(Y) ** 2).sum(-1) / D ** 2, rtol=1e-12, atol=0)
    # the restatement's FFT is the sum of the definition, with the host's twiddle table
    tw = M.twiddle(D)
    k, t = 3, np.arange(D)
    direct = (d[0, 0] * (tw[(k * t) % D, 0] - 1j * tw[(k * t) % D, 1])).sum()
    assert abs(direct - Y[0, 0, k - 1]) <= 1e-13 * np.abs(d[0, 0]).sum()
    assert np.array_equal(modspec.twiddle(D), tw) or np.abs(modspec.twiddle(D) - tw).max() <= 2 ** -52
    assert np.allclose(modspec.frequencies(D), M.frequencies(D), rtol=1e-15)


def test_identities_of_the_postfilter():
    w = _windows(1)
    other = _windows(2)
    mu_n, sg_n = M.window_stats(w, rounded=False)
    mu_g, sg_g = M.window_stats(other, rounded=False)
    y0, tol0 = M.filter_windows(w, mu_n, sg_n, mu_g, sg_g, 0.0)
    assert np.array_equal(y0, w.astype(F64)) and not tol0.any(), "alpha = 0: the input"
    same, _ = M.filter_windows(w, mu_n, sg_n, mu_n, sg_n, 1.0)
    assert np.abs(same - w).max() <= 1e-12, "generated == natural: the identity"
    half, _ = M.filter_windows(w, mu_n, sg_n, mu_n, sg_n, 0.5)
    assert np.abs(half - w).max() <= 1e-12


def test_a_constant_offset_scales_every_component():
    w = _windows(3)
    mu, sg = M.window_stats(w, rounded=False)
    delta = 0.8
    y, _ = M.filter_windows(w, mu + delta, sg, mu, sg, 1.0)
    mean, d, _ = M.analyse(w)
    assert np.abs(y - (mean[..., None] + math.exp(delta / 2) * d)).max() <= 1e-12
    # half the strength: half the log-gain
    y, _ = M.filter_windows(w, mu + delta, sg, mu, sg, 0.5)
    assert np.abs(y - (mean[..., None] + math.exp(delta / 4) * d)).max() <= 1e-12


def test_the_gain_clamp_holds():
    w = _windows(4)
    mu, sg = M.window_stats(w, rounded=False)
    mean, d, Y = M.analyse(w)
    for db in (12.0, 3.0):
        cap = math.exp(M.max_log_gain(db))
        assert abs(20 * math.log10(cap) - db) < 1e-12
        for sign in (1.0, -1.0):
            y, _ = M.filter_windows(w, mu + sign * 50.0, sg, mu, sg, 1.0, max_gain_db=db)
            assert np.abs(y - (mean[..., None] + cap ** sign * d)).max() <= 1e-12, "an offset far beyond the clamp: the clamp"
        y, _ = M.filter_windows(w, mu, 30.0 * sg, mu, sg, 1.0, max_gain_db=db)
        _, _, Y2 = M.analyse(y)
        g = np.abs(Y2) / np.abs(Y)
        assert g.max() <= cap * (1 + 1e-9) and g.min() >= (1 - 1e-9) / cap and g.max() > 0.99 * cap


def test_restoration_of_a_known_attenuation():
    rng = np.random.RandomState(5)
    D, C, n = 16, 3, 12
    nat = M.trajectories(rng, (n, C, D)).astype(F64)
    a = rng.uniform(0.3, 1.0, D // 2)
    gen = M.attenuate(nat, a)
    mean_n, _, N = M.analyse(nat)
    _, _, G = M.analyse(gen)
    assert np.abs(G - a * N).max() <= 1e-12
    stats_n, stats_g = M.window_stats(nat, rounded=False), M.window_stats(gen, rounded=False)
    assert np.abs(stats_g[0] - stats_n[0] - 2 * np.log(a)).max() <= 1e-12 and np.abs(stats_g[1] - stats_n[1]).max() <= 1e-10
    back, _ = M.filter_windows(gen, *stats_n, *stats_g, 1.0)
    assert np.abs(back - nat).max() <= 1e-9, "alpha = 1 returns the natural windows"
    part, _ = M.filter_windows(gen, *stats_n, *stats_g, 0.5)
    _, _, P = M.analyse(part)
    assert np.abs(P - np.sqrt(a) * N).max() <= 1e-9, "alpha = 0.5: half the way in the log domain"
    # hop = D, L a multiple of D: the windows are the utterance's own blocks and come back as the utterance
    utt_n = [np.concatenate(list(nat[:5]), 1), np.concatenate(list(nat[5:]), 1)]
    utt_g = [np.concatenate(list(gen[:5]), 1), np.concatenate(list(gen[5:]), 1)]
    assert utt_n[0].shape == (C, 5 * D) and 0.0 <= min(u.min() for u in utt_n) and max(u.max() for u in utt_n) <= 1.0
    res = M.postfilter(utt_g, D, D, *stats_n, *stats_g, 1.0)
    for (ref, _), want in zip(res, utt_n):
        assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-9
    # and the scores say so: the generated set is smoother, the restored one is not
    lnv = lambda us: np.mean([np.log(u.var(1)) for u in us], 0)
    sc = M.score(stats_g[0], lnv(utt_g), stats_n[0], lnv(utt_n))
    assert sc["gv_ratio_db"] < -0.5 and sc["msd_db"] > 1.0
    assert np.allclose(sc["profile"], 2 * np.log(a), atol=1e-12)
    back_stats = M.window_stats(back, rounded=False)
    assert M.score(back_stats[0], lnv([r for r, _ in res]), stats_n[0], lnv(utt_n))["msd_db"] < 1e-8


def test_short_utterances_and_alpha_zero_keep_their_bits_in_the_restatement():
    rng = np.random.RandomState(6)
    D = 8
    mels = [M.trajectories(rng, (2, L)) for L in M.case_lengths(D)]
    mu, sg = M.window_stats(M.trajectories(rng, (9, 2, D)))
    mu_g, sg_g = M.window_stats(M.trajectories(rng, (9, 2, D)))
    for (ref, tol), m in zip(M.postfilter(mels, D, D // 2, mu, sg, mu_g, sg_g, 0.0), mels):
        assert np.array_equal(ref, m.astype(F64)) and not tol.any()
    res = M.postfilter(mels, D, D // 2, mu, sg, mu_g, sg_g, 1.0)
    assert np.array_equal(res[0][0], mels[0].astype(F64)) and not res[0][1].any(), "L = D - 1: no window, the input's bits"
    for (ref, tol), m in zip(res[1:], mels[1:]):
        assert ref.shape == m.shape and (tol > 0).all() and ref.min() >= 0.0 and ref.max() <= 1.0
        assert np.abs(ref - m).max() > 1e-3


def test_bounds_are_what_the_formats_give():
    w = _windows(7, 6, 2, 64)
    r = M.modspec(w)
    assert (r["ratio"] >= M.MIN_RATIO).all()
    assert (r["tol_s"] <= 2 * 64 * 2.0 ** -53 * 1.0001 / M.MIN_RATIO + 2.0 ** -24 * np.abs(r["s"])).all()
    assert (r["tol_s"] >= 2.0 ** -24 * np.abs(r["s"])).all()
    y, tol = M.filter_windows(w, *M.window_stats(w), *M.window_stats(_windows(8, 6, 2, 64)), 1.0)
    assert (tol < 2.0 ** -23 * np.maximum(np.abs(y), 1e-3)).all(), "the filter's bound is little more than the fp32 store"


# ------------------------------------------------------------------------------------------------------------- host side
def test_plan_gives_short_utterances_no_window():
    D = 8
    p = modspec.plan(M.case_lengths(D), D, D // 2)
    utt, win, ld, n = M.cut(M.case_lengths(D), D, D // 2)
    assert np.array_equal(p["utt"], utt) and np.array_equal(p["win"], win) and (p["ld"], p["nwin"]) == (ld, n)
    assert p["utt"][0].tolist() == [0, 7, 0, 0] and p["win"][0].tolist() == [-1, 0] and p["nwin"] == len(p["win"]) - 1
    for D_, hop in ((7, None), (6, None), (130, None), (8, 0), (8, 9)):
        with pytest.raises(ValueError):
            modspec.check_window(D_, hop)
    assert modspec.check_window(64) == (64, 32) and modspec.check_window(10, 10) == (10, 10)
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    defs = dict(re.findall(r"^#define (DVAE_MODSPEC_[A-Z0-9_]+) (\S+)$", hdr, flags=re.M))
    assert defs == {"DVAE_MODSPEC_DMIN": "8", "DVAE_MODSPEC_DMAX": "128", "DVAE_MODSPEC_FLOOR": "1e-30",
                    "DVAE_MODSPEC_SIGMA_MIN": "1e-6"}
    assert (modspec.D_MIN, modspec.D_MAX, modspec.FLOOR, modspec.SIGMA_MIN) == (M.D_MIN, M.D_MAX, M.FLOOR, M.SIGMA_MIN) == \
        (8, 128, 1e-30, 1e-6)


def _stats_of(groups, D=16, hop=8):
    """ModSpecStats from the restatement: {name: [mel [C, L], ...]}"""
    r = M.group_stats(groups, D, hop)
    return modspec.ModSpecStats(*(r[k] for k in ("names", "D", "hop", "s_sum", "s_sq", "windows", "v_sum", "lnv_sum", "utterances")))


def test_stats_container_round_trip_merge_and_refusals(tmp_path):
    rng = np.random.RandomState(9)
    mel = lambda L: M.trajectories(rng, (3, L))
    a = {"x": [mel(40), mel(9), mel(16)], "y": [mel(33)]}
    b = {"y": [mel(50)], "z": [mel(21), mel(17)]}
    sa, sb = _stats_of(a), _stats_of(b)
    assert sa.windows.tolist() == [4 + 1, 4] and sa.utterances.tolist() == [2, 1], "the 9-frame utterance enters nothing"
    path = sa.save(tmp_path / "stats")
    assert path.endswith(".npz")
    back = modspec.ModSpecStats.load(path)
    assert (back.names, back.D, back.hop) == (sa.names, 16, 8)
    for k in ("s_sum", "s_sq", "windows", "v_sum", "lnv_sum", "utterances"):
        got, want = getattr(back, k), getattr(sa, k)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), k
    both = sa.merge(sb)
    union = _stats_of({"x": a["x"], "y": a["y"] + b["y"], "z": b["z"]})
    assert both.names == ["x", "y", "z"] and both.windows.tolist() == union.windows.tolist()
    for k in ("s_sum", "s_sq", "v_sum", "lnv_sum", "utterances"):
        got, want = getattr(both, k), getattr(union, k)
        assert np.array_equal(got[[0, 2]], want[[0, 2]]), k                # a group one side holds: taken over
        assert np.allclose(got[1], want[1], rtol=1e-13, atol=0), k         # both hold y: (a's sum) + (b's sum), another association
    mu, sg = M.mu_sigma(sa.s_sum[0], sa.s_sq[0], sa.windows[0])
    assert np.array_equal(sa.mean("x"), mu) and np.array_equal(sa.std("x"), sg) and (sa.std("x") >= M.SIGMA_MIN).all()
    assert np.array_equal(sa.gv("x"), sa.v_sum[0] / 2) and sa.mean("x").shape == (3, 8) and sa.gv("x").shape == (3,)
    sc = modspec.score_stats(sa, "x", sb, "z")
    ref = M.score(sa.mean("x"), sa.log_gv("x"), sb.mean("z"), sb.log_gv("z"))
    assert sc["msd_db"] == pytest.approx(ref["msd_db"], rel=1e-14) and sc["gv_ratio_db"] == pytest.approx(ref["gv_ratio_db"], rel=1e-12)
    assert np.allclose(sc["profile"], ref["profile"], rtol=0, atol=1e-15) and np.allclose(sc["frequencies_hz"], M.frequencies(16))
    with pytest.raises(ValueError, match="D=16"):
        sa.merge(_stats_of(b, D=8, hop=4))
    with pytest.raises(ValueError):
        modspec.score_stats(sa, "x", _stats_of(b, D=8, hop=4), "z")
    with pytest.raises(KeyError):
        sa.mean("nobody")
    empty = _stats_of({"short": [mel(9)]})
    with pytest.raises(ValueError, match="no window"):
        empty.mean("short")
    with pytest.raises(ValueError):
        modspec.ModSpecStats(["x"], 7, None, sa.s_sum[:1], sa.s_sq[:1], [1], sa.v_sum[:1], sa.lnv_sum[:1], [1])


# --------------------------------------------------------------------------------------------------------------- commands
@pytest.mark.parametrize("extra,what", [(["--ms-postfilter", "0"], "--ms-postfilter"), (["--ms-postfilter", "1.5"], "--ms-postfilter"),
                                        (["--ms-postfilter", "nan"], "--ms-postfilter"),
                                        (["--ms-postfilter", "0.5", "--ms-window", "7"], "--ms-window"),
                                        (["--ms-postfilter", "0.5", "--ms-window", "130"], "--ms-window"),
                                        (["--ms-postfilter", "0.5", "--ms-max-gain-db", "0"], "--ms-max-gain-db")])
def test_convert_refuses_illegal_postfilter_flags(extra, what, capsys):
    assert convert.main(["--log_dir", "nowhere", "--source", "a.wav", "--target", "b.wav"] + extra) == 2
    assert what in capsys.readouterr().err


def test_score_command_argument_errors(tmp_path, capsys):
    assert modspec.main(["score", str(tmp_path), str(tmp_path), "--D", "7"]) == 2
    assert "D=7" in capsys.readouterr().err
    assert modspec.main(["score", str(tmp_path / "missing"), str(tmp_path)]) == 2
    assert "not a directory" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        modspec.main(["score", str(tmp_path)])
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        modspec.main(["rate", str(tmp_path), str(tmp_path)])
    assert e.value.code == 2


def test_abi_number_and_bindings():
    from dvae_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dvae_hip.h")).read()
    assert int(re.search(r"#define DVAE_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 319
    for name, n in (("dvae_mel_gv", 7), ("dvae_modspec_windows", 7), ("dvae_modspec_group_sum", 10), ("dvae_modspec_filter", 13)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
        assert re.search(r"\bint %s\(" % name, hdr)
