"""F0 tracking and the log-F0 RMSE along the MCD alignment on the GPU (dvae_amd.evaluate): the Viterbi
kernel against the float64 restatement of tests/test_f0.py fed the GPU's own autocorrelation, flags and gain; the smallest
shapes at which it can go wrong; batch independence and determinism; the DTW kernel with the log-F0 payload against the
plain one (bit for bit) and the float64 payload restatement; the score end to end; and the CLI with and without --f0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from dvae_amd import evaluate as ev  # noqa: E402
from test_f0 import (dtw_payload_ref, local_scores, path_objective, pitch_signals, runs_of,  # noqa: E402
                     track_ref)
from test_mcd import harmonic, write_pcm16  # noqa: E402


@pytest.fixture(scope="module")
def fe():
    return ev.MelCepstrum()


def _host(out):
    """the tracker's inputs and outputs of one packed batch as numpy"""
    import torch
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("r", "voiced", "lag", "f0", "lf0v")}


def _check_against_float64(r, gain, voiced, lag, f0, name=""):
    """one utterance: the GPU path's objective within 1e-9 of the float64 optimum on every run (sums of at most 8192 terms
    of magnitude <= 3 in float64 err below 1e-11); where the optimum's final margin is >= 1e-4 the lags are equal on every
    frame of the run; f0 within 1e-6 relative wherever the lags are equal; 0 on unvoiced frames"""
    voiced = voiced.astype(bool)
    ref = track_ref(r[:, :207], gain[:207], voiced)
    l2 = ev.f0_tables()[0]
    assert np.all(lag[~voiced] == 0) and np.all(f0[~voiced] == 0.0), name
    assert np.all((lag[voiced] >= ev.LAG_MIN) & (lag[voiced] <= ev.LAG_MAX)), name
    st = lag.astype(np.int64) - ev.LAG_MIN
    sure = 0
    for n, (a, b) in enumerate(runs_of(voiced)):
        s = local_scores(r[a:b + 1, :207], gain[:207])
        got = path_objective(s, l2, st[a:b + 1])
        print(f"{name} run {a}..{b}: objective {got:.12f}, float64 optimum {ref['objective'][n]:.12f}, "
              f"final margin {ref['margin'][n]:.3e}")
        assert abs(got - ref["objective"][n]) <= 1e-9, (name, a, b, got, ref["objective"][n])
        if ref["margin"][n] >= 1e-4:
            sure += 1
            assert np.array_equal(st[a:b + 1], ref["state"][a:b + 1]), (name, a, b)
    same = voiced & (st == ref["state"])
    assert np.all(np.abs(f0[same] - ref["f0"][same]) <= 1e-6 * ref["f0"][same]), name
    return sure


# --------------------------------------------------------------------------------------------------------- Viterbi
def test_viterbi_matches_float64_on_tones_and_chirps(fe):
    sigs = pitch_signals()
    out = fe.packed([x for _, x, _ in sigs], f0=True)
    h = _host(out)
    gain = fe.gain.cpu().numpy()
    sure = 0
    for (name, x, truth), (r0, M), k in zip(sigs, out["table"][:, :2], out["count"]):
        sl = slice(r0, r0 + M)
        sure += _check_against_float64(h["r"][sl], gain, h["voiced"][sl], h["lag"][sl], h["f0"][sl], name)
        v = h["voiced"][sl].astype(bool)
        inner = np.nonzero(v)[0]
        inner = inner[(inner >= 4) & (inner < M - 4)]
        err = 1200.0 * np.abs(np.log2(h["f0"][sl][inner].astype(np.float64) / truth[inner]))
        assert err.max() <= 50.0, (name, err.max())
        # lf0v: ln f0 of the k-th voiced frame at row0 + k, the row its coefficients have in feats
        assert k == v.sum()
        want = np.log(h["f0"][sl][v].astype(np.float64))
        assert np.all(np.abs(h["lf0v"][r0:r0 + k] - want) <= 1e-6), name
    assert sure >= len(sigs) - 1, sure               # the margin condition holds on (nearly) all of these signals


def test_viterbi_short_runs_chunk_boundary_and_an_unvoiced_utterance(fe):
    """the kernel on flags set by hand over a tone's autocorrelation: runs of 1 and 2 frames, a run over the 256-frame
    boundary of the traceback, a run that ends on the utterance's last frame; and an utterance without a voiced frame,
    for which lag and f0 are 0 and lf0v is not written"""
    import torch
    from dvae_amd.packed import upload
    tone = harmonic(23999, 140.0, seed=31)            # 300 frames
    out = fe.packed([tone, np.zeros(4000, np.float32)])
    M = int(out["table"][0, 1])
    assert M == 300
    rows = int(out["table"][:, 1].sum())
    flags = np.zeros(rows, np.int32)
    flags[5] = 1
    flags[10:12] = 1
    flags[20:291] = 1
    flags[299] = 1
    segs = upload(out["table"], fe.device, np.int64)
    bufs = dict(lag=torch.full((rows,), 7, device=fe.device, dtype=torch.int32),
                f0=torch.full((rows,), 7.0, device=fe.device, dtype=torch.float32),
                lf0v=torch.full((rows,), 7.0, device=fe.device, dtype=torch.float32))
    got = fe.f0_viterbi(out["r"], torch.from_numpy(flags).to(fe.device), segs, 2, rows, out=bufs)
    torch.cuda.synchronize()
    lag, f0, lf0v = (got[k].cpu().numpy() for k in ("lag", "f0", "lf0v"))
    r, gain = out["r"].cpu().numpy(), fe.gain.cpu().numpy()
    assert _check_against_float64(r[:M], gain, flags[:M], lag[:M], f0[:M], "hand-set flags") == 4
    nv = int(flags.sum())
    assert np.all(np.abs(lf0v[:nv] - np.log(f0[:M][flags[:M] > 0].astype(np.float64))) <= 1e-6)
    assert np.all(lf0v[nv:] == 7.0)                   # one writer per voiced frame, nothing else touched
    assert np.all(lag[M:] == 0) and np.all(f0[M:] == 0.0)
    interior = np.arange(24, 287)
    assert np.all(1200 * np.abs(np.log2(f0[interior] / 140.0)) < 50.0)


def test_viterbi_runs_do_not_see_each_other(fe):
    """tone / digital silence / tone in one utterance: the second run starts from its own local score (D = s at its first
    frame), as the restatement does run by run, and lands on the second tone's pitch"""
    x = np.concatenate([harmonic(4000, 120.0, seed=1), np.zeros(2400, np.float32), harmonic(4000, 300.0, seed=2)])
    out = fe.packed([x], f0=True)
    h = _host(out)
    v = h["voiced"].astype(bool)
    runs = runs_of(v)
    assert len(runs) == 2 and not v[60:75].any()
    _check_against_float64(h["r"], fe.gain.cpu().numpy(), h["voiced"], h["lag"], h["f0"], "tone/silence/tone")
    a, b = runs[1]
    s = local_scores(h["r"][a:a + 1, :207], fe.gain.cpu().numpy()[:207])
    alone = track_ref(h["r"][a:b + 1, :207], fe.gain.cpu().numpy()[:207], np.ones(b - a + 1, bool))
    assert h["lag"][a] - ev.LAG_MIN == alone["state"][0]
    print(f"second run's first frame: lag {h['lag'][a]}, arg-max of its own s {ev.LAG_MIN + int(np.argmax(s[0]))}")
    assert np.all(1200 * np.abs(np.log2(h["f0"][a + 4:b - 3] / 300.0)) < 50.0)
    assert np.all(1200 * np.abs(np.log2(h["f0"][4:runs[0][1] - 3] / 120.0)) < 50.0)


def test_viterbi_batch_independence_and_determinism(fe):
    import torch
    rs = np.random.RandomState(32)
    sigs = [harmonic(8000, 100.0, seed=3), pitch_signals()[6][1], np.zeros(3000, np.float32),
            np.concatenate([harmonic(4000, 120.0, seed=1), (0.05 * rs.randn(2400)).astype(np.float32),
                            harmonic(4000, 300.0, seed=2)]), harmonic(333, 400.0, seed=4)]
    out = fe.packed(sigs, f0=True)
    again = fe.packed(sigs, f0=True)
    torch.cuda.synchronize()
    for k in ("lag", "f0"):
        assert torch.equal(out[k], again[k]), k
    lag, f0, lf0v = (out[k].cpu().numpy() for k in ("lag", "f0", "lf0v"))
    lf0v2 = again["lf0v"].cpu().numpy()
    for s, x in enumerate(sigs):
        one = fe.packed([x], f0=True)
        r0, M = out["table"][s, :2]
        k = out["count"][s]
        assert one["count"][0] == k
        assert np.array_equal(one["lag"].cpu().numpy(), lag[r0:r0 + M])
        assert np.array_equal(one["f0"].cpu().numpy().view(np.int32), f0[r0:r0 + M].view(np.int32))
        assert np.array_equal(one["lf0v"].cpu().numpy()[:k].view(np.int32), lf0v[r0:r0 + k].view(np.int32))
        assert np.array_equal(lf0v2[r0:r0 + k].view(np.int32), lf0v[r0:r0 + k].view(np.int32))
    per = fe.f0_batch(sigs)
    assert [len(f) for f, _ in per] == [ev.frame_count(len(x)) for x in sigs]
    assert all(np.array_equal(f > 0, v) for f, v in per) and not per[2][1].any()


def test_packed_without_f0_is_unchanged(fe):
    x = harmonic(8000, 150.0, seed=5)
    plain, with_f0 = fe.packed([x]), fe.packed([x], f0=True)
    assert set(with_f0) - set(plain) == {"lag", "f0", "lf0v"}
    assert set(plain) == {"table", "feats", "count", "mc", "voiced", "peak", "r"}
    for k in ("feats", "mc", "voiced", "peak", "r"):
        assert np.array_equal(plain[k].cpu().numpy()[:plain["count"][0] if k == "feats" else None],
                              with_f0[k].cpu().numpy()[:plain["count"][0] if k == "feats" else None]), k


# ------------------------------------------------------------------------------------------------------------- DTW
DTW_SHAPES = [(1, 1), (1, 300), (300, 1), (37, 300), (300, 37), (1500, 1200), (4500, 4096)]


def test_dtw_f0_is_the_dtw_plus_the_payload():
    """cost and length bit-identical to dvae_dtw_batch; sse against the float64 restatement to 1e-3 relative (a plain
    fp32 running sum of <= 8191 non-negative terms is within 8191 * 2^-24 = 4.9e-4 of the exact sum)"""
    rs = np.random.RandomState(40)
    xs = [rs.randn(n, ev.DIM).astype(np.float32) for n, _ in DTW_SHAPES]
    ys = [rs.randn(m, ev.DIM).astype(np.float32) for _, m in DTW_SHAPES]
    lxs = [rs.uniform(4.2, 6.7, n).astype(np.float32) for n, _ in DTW_SHAPES]
    lys = [rs.uniform(4.2, 6.7, m).astype(np.float32) for _, m in DTW_SHAPES]
    cost, length, sse = ev.dtw_batch_f0(xs, ys, lxs, lys)
    c0, l0 = ev.dtw_batch(xs, ys)
    assert np.array_equal(cost.view(np.int64), c0.view(np.int64)) and np.array_equal(length, l0)
    assert sse.dtype == np.float64
    for p, shape in enumerate(DTW_SHAPES):
        c, l, want = dtw_payload_ref(xs[p], ys[p], lxs[p], lys[p])
        print(f"{shape}: sse {sse[p]:.6f}, float64 {want:.6f}, relative error {abs(sse[p] - want) / want:.2e}")
        assert length[p] == l, (shape, length[p], l)
        assert abs(sse[p] - want) <= 1e-3 * want, (shape, sse[p], want)
    # one pair alone: the same bits
    c1, l1, s1 = ev.dtw_batch_f0(xs[3:4], ys[3:4], lxs[3:4], lys[3:4])
    assert c1.view(np.int64)[0] == cost.view(np.int64)[3] and l1[0] == length[3] and s1[0] == sse[3]


def test_dtw_f0_empty_and_oversize():
    import torch
    from dvae_amd._lib import lib
    rs = np.random.RandomState(41)
    seq = lambda n: rs.randn(n, ev.DIM).astype(np.float32)
    lf = lambda n: rs.uniform(4.2, 6.7, n).astype(np.float32)
    cost, length, sse = ev.dtw_batch_f0([seq(0), seq(5), seq(4)], [seq(9), seq(5), seq(0)], [lf(0), lf(5), lf(4)],
                                        [lf(9), lf(5), lf(0)])
    assert np.isnan(cost[0]) and length[0] == 0 and np.isnan(sse[0]) and np.isnan(sse[2]) and length[2] == 0
    assert np.isfinite(cost[1]) and np.isfinite(sse[1]) and sse[1] >= 0
    big = seq(ev.DTW_MAX_SHORT + 1)
    with pytest.raises(ValueError, match="DTW kernel supports"):
        ev.dtw_batch_f0([big], [big], [lf(len(big))], [lf(len(big))])
    n = ev.DTW_MAX_SHORT + 1
    x = torch.zeros((n, ev.DIM), device="cuda")
    l = torch.zeros(n, device="cuda")
    pairs = np.array([[0, n, 0, n]], dtype=np.int64)
    pd = torch.from_numpy(pairs).cuda()
    out_c = torch.full((1,), 7.0, device="cuda", dtype=torch.float64)
    out_l = torch.full((1,), 7, device="cuda", dtype=torch.int64)
    out_s = torch.full((1,), 7.0, device="cuda", dtype=torch.float64)
    rc = lib().dvae_dtw_batch_f0(x.data_ptr(), x.data_ptr(), l.data_ptr(), l.data_ptr(), pd.data_ptr(), pairs.ctypes.data,
                                 1, out_c.data_ptr(), out_l.data_ptr(), out_s.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and out_c.item() == 7.0 and out_l.item() == 7 and out_s.item() == 7.0


# ------------------------------------------------------------------------------------------------------ end to end
def _pair_signals():
    rs = np.random.RandomState(42)
    a = [harmonic(20000, 120.0, seed=20), harmonic(16000, 200.0, seed=21)]
    b = [harmonic(22000, 150.0, seed=23), (harmonic(16000, 210.0, seed=24) + 0.05 * rs.randn(16000)).astype(np.float32)]
    return a, b


def test_score_end_to_end(fe):
    a, b = _pair_signals()
    plain = ev.mcd_batch(a, b, features=fe)
    res = ev.mcd_batch(a, b, features=fe, f0=True)
    assert set(res) - set(plain) == {"lf0_rmse", "lf0_rmse_cents", "lf0_mean_converted", "lf0_std_converted",
                                     "lf0_mean_reference", "lf0_std_reference", "mean_lf0_rmse_cents",
                                     "lf0_pooled_mean_converted", "lf0_pooled_std_converted", "lf0_pooled_mean_reference",
                                     "lf0_pooled_std_reference"}
    for k in ("mcd", "cost"):
        assert np.array_equal(res[k].view(np.int64), plain[k].view(np.int64)), k
    assert np.array_equal(res["path_length"], plain["path_length"]) and res["mean_mcd"] == plain["mean_mcd"]
    # 8-harmonic tones at 120 and 150 Hz: a major third apart on every cell of the path
    want = 1200.0 * np.log2(1.25)
    print(f"120 Hz against 150 Hz: {res['lf0_rmse_cents'][0]:.3f} cents, 1200 log2(1.25) = {want:.3f}")
    assert abs(res["lf0_rmse_cents"][0] - want) <= 5.0, res["lf0_rmse_cents"][0]
    assert np.allclose(res["lf0_rmse_cents"], ev.CENTS_PER_NAT * res["lf0_rmse"], rtol=1e-15)
    assert abs(np.exp(res["lf0_mean_converted"][0]) - 120.0) < 1.0 and abs(np.exp(res["lf0_mean_reference"][0]) - 150.0) < 1.0
    assert np.all(res["lf0_std_converted"] < 0.02)
    assert np.isclose(res["mean_lf0_rmse_cents"], res["lf0_rmse_cents"].mean(), rtol=1e-15)
    # pooled over all voiced frames of a side: between the two files' means, the spread that of 120 against 200 Hz
    lo, hi = sorted(res["lf0_mean_converted"])
    assert lo < res["lf0_pooled_mean_converted"] < hi
    assert abs(res["lf0_pooled_std_converted"] - np.log(200.0 / 120.0) / 2) < 0.02
    # identical waveforms, and the pair the other way round
    same = ev.mcd_batch(a, a, features=fe, f0=True)
    assert np.all(same["lf0_rmse"] == 0.0) and np.all(same["mcd"] == 0.0) and same["mean_lf0_rmse_cents"] == 0.0
    rev = ev.mcd_batch(b, a, features=fe, f0=True)
    assert np.all(np.abs(res["lf0_rmse"] - rev["lf0_rmse"]) <= 1e-5 * res["lf0_rmse"]), (res["lf0_rmse"], rev["lf0_rmse"])
    assert np.array_equal(res["lf0_mean_converted"], rev["lf0_mean_reference"])
    # a side without voiced frames: NaN wherever the MCD is
    nan = ev.mcd_batch([a[0], np.zeros(8000, np.float32)], [np.zeros(4000, np.float32), a[1]], features=fe, f0=True)
    assert np.all(np.isnan(nan["mcd"])) and np.all(np.isnan(nan["lf0_rmse"])) and np.isnan(nan["mean_lf0_rmse_cents"])
    assert np.isnan(nan["lf0_mean_reference"][0]) and np.isfinite(nan["lf0_mean_converted"][0])
    assert np.isfinite(nan["lf0_pooled_mean_converted"]) and np.isfinite(nan["lf0_pooled_std_reference"])


# ------------------------------------------------------------------------------------------------------------- CLI
def _run(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "dvae_amd.evaluate"] + [str(a) for a in args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_cli_with_and_without_f0(tmp_path):
    a, b = _pair_signals()
    cdir, rdir = tmp_path / "p225_to_p226", tmp_path / "p226"
    cdir.mkdir()
    rdir.mkdir()
    for u, x, y in (("001", a[0], b[0]), ("002", a[1], b[1])):
        write_pcm16(cdir / f"convert_p225_to_p226_{u}.wav", x)
        write_pcm16(rdir / f"p226_{u}.wav", y)
    # without --f0: stdout and mcd.json as they were
    p = _run([cdir, rdir])
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("utterance 001 mcd: ") and lines[1].startswith("utterance 002 mcd: ")
    assert lines[-1].startswith("mean mcd: ")
    plain = json.loads((cdir / "mcd.json").read_text())
    assert set(plain) == {"converted_dir", "reference_dir", "pairs", "mean_mcd", "scored", "no_voiced", "unmatched"}
    row_keys = {"utterance", "converted", "reference", "mcd", "path_length", "frames_converted", "frames_reference",
                "voiced_converted", "voiced_reference"}
    assert all(set(r) == row_keys for r in plain["pairs"]) and plain["scored"] == 2
    for r, line in zip(plain["pairs"], lines):
        assert float(line.split("mcd: ")[1]) == r["mcd"] and r["mcd"] > 0
    # with it: the mcd lines first and unchanged, then the lf0 lines, `mean mcd` last
    out = tmp_path / "f0.json"
    q = _run([cdir, rdir, "--f0", "--json", out])
    assert q.returncode == 0, q.stdout + q.stderr
    fl = q.stdout.strip().splitlines()
    assert fl[:2] == lines[:2] and fl[-1] == lines[-1] and len(fl) == 6
    assert fl[2].startswith("utterance 001 lf0 rmse: ") and fl[3].startswith("utterance 002 lf0 rmse: ")
    assert " cents (converted mean " in fl[2] and " Hz, reference mean " in fl[2] and fl[2].endswith(" Hz)")
    assert fl[4].startswith("mean lf0 rmse: ")
    res = json.loads(out.read_text())
    assert set(res) == set(plain) | {"mean_lf0_rmse_cents", "lf0_pooled_mean_converted", "lf0_pooled_std_converted",
                                     "lf0_pooled_mean_reference", "lf0_pooled_std_reference"}
    for r, r0, line in zip(res["pairs"], plain["pairs"], fl[2:4]):
        assert {k: r[k] for k in row_keys} == r0
        assert set(r) == row_keys | {"lf0_rmse", "lf0_rmse_cents", "lf0_mean_converted", "lf0_std_converted",
                                     "lf0_mean_reference", "lf0_std_reference"}
        assert np.isfinite(r["lf0_rmse_cents"]) and r["lf0_rmse_cents"] > 0
        assert float(line.split("lf0 rmse: ")[1].split(" cents")[0]) == r["lf0_rmse_cents"]
    assert np.isclose(res["mean_lf0_rmse_cents"], np.mean([r["lf0_rmse_cents"] for r in res["pairs"]]), rtol=1e-12)
    assert abs(res["pairs"][0]["lf0_rmse_cents"] - 1200 * np.log2(1.25)) <= 5.0
