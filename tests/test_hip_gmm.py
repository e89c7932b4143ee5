"""The GMM-UBM kernels of csrc/probe.hip (dvae_gmm_estep, dvae_gmm_score) on the MI355X through the C
ABI, against the float64 restatement of tests/gmm_ref.py, and dvae_amd.verify above them.

lse and gamma are held to the two bounds derived in gmm_ref (from eps32 = 2^-24 and the operation counts, not from what the
kernel gives), the float64 statistics to the summation bound against the GPU's OWN gamma and lse, and what the contract
calls bit-exact is compared bit for bit: K = 1, two calls, null outputs, the scorer against the E-step's lse in the scorer's
order, a batch against single launches, M models against one at a time.  Every buffer a launch may write is a guarded one
of tests/kernel_harness.py, pre-filled with 0xFF; inputs carry NaN wherever the entry point must not read.  The worst
error / bound per shape is printed at the module's end.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import assert_same_bits, Buf, EINVAL, F32, F64, guards, ibuf, L, ok, Pad, st, Worst
import dvae_amd  # noqa: E402,F401
import gmm_ref as G  # noqa: E402
from test_gmm_ref import margin_and_bound  # noqa: E402
from test_mcd import write_pcm16  # noqa: E402

WORST = Worst("test_hip_gmm.py (rows: K, D, ldx, col0)")
note = WORST.note
SHAPES = [(1, 1, 1, 0), (3, 23, 24, 1), (64, 23, 24, 1), (256, 32, 32, 0), (5, 7, 9, 2)]
# either side of 64, 128 and 256: the frame tiles of K > 128, K <= 128 and K <= 64
NS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def key(K, D, ldx, col0):
    return f"{K},{D},{ldx},{col0}"


def make_model(rs, K, D, tiny_weight=True):
    mu, var = rs.randn(K, D), rs.uniform(0.3, 2.0, (K, D))
    w = np.maximum(rs.dirichlet(np.ones(K)), 1e-4)
    if K > 1 and tiny_weight:
        w[0] = 1e-6                                   # a component of weight 1e-6
    return w / w.sum(), mu, var


def make_frames(rs, N, mu, var, ldx, col0, far=True):
    """[N, ldx] fp32, NaN outside the columns col0 .. col0 + D; frames 0 and 1 lie 50 and 300 standard deviations away
    from every component"""
    K, D = mu.shape
    x = (mu[rs.randint(0, K, N)] + rs.randn(N, D) * np.sqrt(var.mean())).astype(F32)
    if far:
        sd = np.sqrt(var.max())
        x[0] = (np.abs(mu).max() + 50.0 * sd) * np.where(np.arange(D) % 2, -1.0, 1.0)
        if N > 1:
            x[1] = np.abs(mu).max() + 300.0 * sd
    full = np.full((N, ldx), np.nan, F32)
    full[:, col0:col0 + D] = x
    return x, full


class Tables:
    def __init__(self, models):
        tabs = [G.tables(*m) for m in models]
        self.host = tabs
        self.a, self.mu, self.prec = (Pad(np.stack([t[i] for t in tabs])) for i in range(3))
        self.K, self.D, self.M = tabs[0][1].shape[0], tabs[0][1].shape[1], len(tabs)


def ws_buf(N, K, D):
    need = L().dvae_gmm_ws_bytes(N, K, D)
    assert need > 0 and need % 8 == 0
    b = Buf((need + 512,), torch.uint8)
    b.slack_from = need
    return b


def estep(full, ldx, col0, N, t, want_lse=True, want_gamma=True, xin=None):
    xin = Pad(full) if xin is None else xin
    lse = Buf((N,)) if want_lse else None
    gamma = Buf((N, t.K)) if want_gamma else None
    ws, stats = ws_buf(N, t.K, t.D), Buf((t.K * (1 + 2 * t.D) + 1,), torch.float64)
    ok(L().dvae_gmm_estep(xin.ptr, ldx, col0, N, t.D, t.a.ptr, t.mu.ptr, t.prec.ptr, t.K, lse.ptr if lse else None,
                          gamma.ptr if gamma else None, ws.ptr, stats.ptr, st()), "dvae_gmm_estep")
    guards(lse, gamma, ws, stats, xin.buf, t.a.buf, t.mu.buf, t.prec.buf)
    return lse, gamma, stats, xin


def score(xin, ldx, col0, segs, t):
    segs = np.ascontiguousarray(segs, np.int64).reshape(-1, 2)
    sb, out = ibuf(segs), Buf((len(segs), t.M), torch.float64)
    ok(L().dvae_gmm_score(xin.ptr, ldx, col0, t.D, sb.ptr, len(segs), t.a.ptr, t.mu.ptr, t.prec.ptr, t.K, t.M, out.ptr,
                          st()), "dvae_gmm_score")
    guards(out, sb)
    return out


# ------------------------------------------------------------------------------------------------------------- E-step
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K,D,ldx,col0", SHAPES)
def test_estep(K, D, ldx, col0, N):
    rs = np.random.RandomState(1000 * K + N)
    model = make_model(rs, K, D)
    x, full = make_frames(rs, N, model[1], model[2], ldx, col0)
    t = Tables([model])
    a, mu, prec = t.host[0]
    lse, gamma, stats, xin = estep(full, ldx, col0, N, t)
    gl, gg, gs = lse.np(), gamma.np(), stats.np()
    _, lse64, g64, q = G.loglik(x, a, mu, prec)
    k = key(K, D, ldx, col0)
    assert np.all(np.isfinite(gl)) and np.all(np.isfinite(gg)), "a frame far from every component must stay finite"
    note((k, "lse"), gl, lse64, G.lse_bound(a, g64, q, D), f"lse N={N}")
    note((k, "gamma"), gg, g64, G.gamma_bound(a, g64, q, D), f"gamma N={N}")
    assert np.all(np.abs(gg.astype(F64).sum(axis=1) - 1.0) <= K * 2.0 ** -23), "posteriors of a frame sum to 1"
    assert lse64[0] < -1e3 * D and (N == 1 or lse64[1] < -3e4 * D)              # the far frames are far
    if K == 1:
        l32, _, _ = G.loglik_f32(x, a, mu, prec)
        assert_same_bits(gg, np.ones((N, 1), F32), "K = 1: every gamma is 1.0f")
        assert_same_bits(gl, l32[:, 0], "K = 1: lse is l_0t")
    # the float64 sums against the GPU's own gamma, lse and x
    n, f, s = G.stats(x, gg)
    an, af, as_ = G.stats_abs(x, gg)
    gn, gf, gs2, glse = G.unpack_stats(gs, K, D)
    note((k, "n"), gn, n, G.sum_bound(N, an) + G.FLOOR, f"n N={N}")
    note((k, "f"), gf, f, G.sum_bound(N, af) + G.FLOOR, f"f N={N}")
    note((k, "s"), gs2, s, G.sum_bound(N, as_) + G.FLOOR, f"s N={N}")
    note((k, "sum lse"), [glse], [gl.astype(F64).sum()], G.sum_bound(N, np.abs(gl.astype(F64)).sum()), f"sum lse N={N}")
    # two calls give the same bits in every output
    lse2, gamma2, stats2, _ = estep(full, ldx, col0, N, t, xin=xin)
    assert np.array_equal(lse2.bits(), lse.bits()) and np.array_equal(gamma2.bits(), gamma.bits())
    assert np.array_equal(stats2.bits(), stats.bits())
    # null lse and gamma: the same statistics
    _, _, stats3, _ = estep(full, ldx, col0, N, t, want_lse=False, want_gamma=False, xin=xin)
    assert np.array_equal(stats3.bits(), stats.bits())
    _, gamma4, stats4, _ = estep(full, ldx, col0, N, t, want_lse=False, xin=xin)
    assert np.array_equal(stats4.bits(), stats.bits()) and np.array_equal(gamma4.bits(), gamma.bits())


def test_estep_many_tiles_per_workgroup():
    """more tiles than workgroups: a workgroup keeps its accumulators across several tiles (K = 130: tiles of 64 frames,
    N = 64 * 512 * 2 + 37 gives 3 tiles per workgroup and a ragged last one)"""
    K, D, ldx, col0 = 130, 3, 4, 1
    N = 64 * 512 * 2 + 37
    rs = np.random.RandomState(5)
    model = make_model(rs, K, D)
    x, full = make_frames(rs, N, model[1], model[2], ldx, col0, far=False)
    t = Tables([model])
    assert L().dvae_gmm_ws_bytes(N, K, D) == 342 * (K * (1 + 2 * D) + 1) * 8      # 1025 tiles, 3 per workgroup
    lse, gamma, stats, xin = estep(full, ldx, col0, N, t)
    gl, gg = lse.np(), gamma.np()
    a, mu, prec = t.host[0]
    _, lse64, g64, q = G.loglik(x, a, mu, prec)
    k = key(K, D, ldx, col0)
    note((k, "lse"), gl, lse64, G.lse_bound(a, g64, q, D), "lse")
    note((k, "gamma"), gg, g64, G.gamma_bound(a, g64, q, D), "gamma")
    n, f, s = G.stats(x, gg)
    an, af, as_ = G.stats_abs(x, gg)
    gn, gf, gs2, glse = G.unpack_stats(stats.np(), K, D)
    note((k, "n"), gn, n, G.sum_bound(N, an) + G.FLOOR, "n")
    note((k, "f"), gf, f, G.sum_bound(N, af) + G.FLOOR, "f")
    note((k, "s"), gs2, s, G.sum_bound(N, as_) + G.FLOOR, "s")
    note((k, "sum lse"), [glse], [gl.astype(F64).sum()], G.sum_bound(N, np.abs(gl.astype(F64)).sum()), "sum lse")
    _, _, stats2, _ = estep(full, ldx, col0, N, t, want_lse=False, want_gamma=False, xin=xin)
    assert np.array_equal(stats2.bits(), stats.bits())


# --------------------------------------------------------------------------------------------------------------- score
@pytest.mark.parametrize("K,D,ldx,col0", SHAPES)
def test_score(K, D, ldx, col0):
    rs = np.random.RandomState(77 + K)
    models = [make_model(rs, K, D, tiny_weight=(m == 0)) for m in range(3)]
    counts = [300, 0, 1, 257, 64]
    N = sum(counts) + 7                                   # rows in front of, and behind, the segments
    x, full = make_frames(rs, N, models[0][1], models[0][2], ldx, col0)
    row0 = 3 + np.concatenate([[0], np.cumsum(counts)[:-1]])
    segs = np.stack([row0, counts], axis=1)
    t3 = Tables(models)
    xin = Pad(full)
    out = score(xin, ldx, col0, segs, t3)
    got = out.np()
    assert np.array_equal(got[1], np.zeros(3)) and not np.signbit(got[1]).any(), "count = 0 gives exactly 0.0"
    k = key(K, D, ldx, col0)
    for m, model in enumerate(models):
        a, mu, prec = t3.host[m]
        _, lse64, g64, q = G.loglik(x, a, mu, prec)
        b = G.lse_bound(a, g64, q, D)
        ref = np.array([lse64[r:r + c].sum() for r, c in segs])
        tol = np.array([b[r:r + c].sum() for r, c in segs]) + G.FLOOR
        note((k, "score"), got[:, m], ref, tol, f"score model {m}")
        # the same bits as the sum of the E-step's own lse over the rows, in the scorer's order
        t1 = Tables([model])
        lse, _, _, _ = estep(full, ldx, col0, N, t1, want_gamma=False, xin=xin)
        gl = lse.np()
        own = np.array([G.score_order_sum(gl[r:r + c]) for r, c in segs])
        assert np.array_equal(got[:, m].view(np.int64), own.view(np.int64)), f"model {m}: not the E-step's lse, summed"
        # M = 3 models against one at a time
        one = score(xin, ldx, col0, segs, t1)
        assert np.array_equal(one.bits()[:, 0], out.bits()[:, m]), f"model {m}: alone and among three"
    # the batch of five against five single launches
    for i in range(len(segs)):
        single = score(xin, ldx, col0, segs[i:i + 1], t3)
        assert np.array_equal(single.bits()[0], out.bits()[i]), f"utterance {i}: alone and in the batch"
    out2 = score(xin, ldx, col0, segs, t3)
    assert np.array_equal(out2.bits(), out.bits())


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    K, D, ldx, col0, N = 5, 7, 9, 2, 40
    rs = np.random.RandomState(3)
    model = make_model(rs, K, D)
    _, full = make_frames(rs, N, model[1], model[2], ldx, col0)
    t, xin = Tables([model]), Pad(full)
    big = Pad(np.zeros((257, 33), F32))
    segs = ibuf(np.array([[0, N]], np.int64))

    def e(x=xin.ptr, ldx=ldx, col0=col0, N=N, D=D, a=t.a.ptr, mu=t.mu.ptr, prec=t.prec.ptr, K=K, ws=True, stats=True):
        lse, gamma, w, s = Buf((40,)), Buf((40, 5)), Buf((1 << 16,), torch.uint8), Buf((5 * 15 + 1,), torch.float64)
        rc = L().dvae_gmm_estep(x, ldx, col0, N, D, a, mu, prec, K, lse.ptr, gamma.ptr, w.ptr if ws else None,
                                s.ptr if stats else None, st())
        assert rc == EINVAL, rc
        guards(lse, gamma, w, s)
        for b in (lse, gamma, w, s):
            assert b.poisoned().all(), "a refused call wrote an output"

    for kw in (dict(x=None), dict(a=None), dict(mu=None), dict(prec=None), dict(ws=False), dict(stats=False), dict(N=0),
               dict(N=-1), dict(K=0), dict(D=0), dict(K=257, a=big.ptr, mu=big.ptr, prec=big.ptr),
               dict(D=33, ldx=40, mu=big.ptr, prec=big.ptr), dict(col0=-1), dict(ldx=col0 + D - 1), dict(ldx=0)):
        e(**kw)

    def s(x=xin.ptr, ldx=ldx, col0=col0, D=D, sg=segs.ptr, nseg=1, a=t.a.ptr, mu=t.mu.ptr, prec=t.prec.ptr, K=K, M=1,
          out=True):
        o = Buf((4, 4), torch.float64)
        rc = L().dvae_gmm_score(x, ldx, col0, D, sg, nseg, a, mu, prec, K, M, o.ptr if out else None, st())
        assert rc == EINVAL, rc
        guards(o)
        assert o.poisoned().all(), "a refused call wrote an output"

    for kw in (dict(x=None), dict(sg=None), dict(a=None), dict(mu=None), dict(prec=None), dict(out=False), dict(nseg=0),
               dict(M=0), dict(K=0), dict(D=0), dict(K=257, a=big.ptr, mu=big.ptr, prec=big.ptr),
               dict(D=33, ldx=40, mu=big.ptr, prec=big.ptr), dict(col0=-1), dict(ldx=col0 + D - 1)):
        s(**kw)
    assert L().dvae_gmm_ws_bytes(0, K, D) == 0 and L().dvae_gmm_ws_bytes(N, 257, D) == 0
    assert L().dvae_gmm_ws_bytes(N, K, 33) == 0


# ---------------------------------------------------------------------------------- the trainer and the verifier, no audio
def test_one_em_step_no_drift_and_the_planted_speakers():
    from dvae_amd import verify
    p = G.planted_speakers(0)
    D, K = p["D"], 8
    x = np.concatenate(p["train"])
    N = len(x)
    feats = torch.from_numpy(x.astype(F32)).cuda().contiguous()
    hist = []
    final, lls = verify.train_ubm(feats, K=K, iters=5, seed=0, col0=0, dim=D, history=hist)
    assert len(hist) == 5 and len(lls) == 5
    _, _, _, idx = G.init_from_frames(x, K, 0)
    assert np.array_equal(hist[0]["model"].mu, x[idx]), "the start: the frames drawn by default_rng(seed)"
    assert np.allclose(hist[0]["gvar"], G.global_variance(x), rtol=1e-12, atol=0)
    params = [h["model"] for h in hist] + [final]
    for i in range(5):
        m, nxt, gvar = params[i], params[i + 1], hist[i]["gvar"]
        a, mu, prec = G.tables(m.w, m.mu, m.var)
        _, lse64, g64, q = G.loglik(x, a, mu, prec)
        n, f, s = G.stats(x, g64)
        assert np.all(n > 4 * (D + 1)), "no component near the starved rule on the planted data"
        gb = G.gamma_bound(a, g64, q, D)
        dn = gb.sum(axis=0) + G.sum_bound(N, n)
        df = gb.T @ np.abs(x) + G.sum_bound(N, np.abs(g64).T @ np.abs(x))
        ds = gb.T @ (x * x) + G.sum_bound(N, g64.T @ (x * x))
        w_ref, mu_ref, var_ref = G.m_step(n, f, s, N, m.mu, m.var, gvar)
        bw, bmu, bvar = G.m_step_bounds(n, f, s, dn, df, ds, N)
        note(("em step", "w"), nxt.w, w_ref, bw, f"w after iteration {i}")
        note(("em step", "mu"), nxt.mu, mu_ref, bmu, f"mu after iteration {i}")
        note(("em step", "var"), nxt.var, var_ref, bvar, f"var after iteration {i}")
        note(("em step", "mean ll"), [lls[i]], [lse64.sum() / N], [G.lse_bound(a, g64, q, D).sum() / N], f"ll {i}")
    # the verifier on the planted speakers: frames uploaded directly
    ubm = (final.w, final.mu, final.var)
    ta = G.tables(*ubm)
    ref_models = []
    for xs in p["train"]:
        n, f, _ = G.stats(xs, G.loglik(xs, *ta)[2])
        ref_models.append(G.map_adapt(*ubm, n, f, len(xs)))
    gap, bound = margin_and_bound(p["test"], ubm, ref_models, D)
    assert gap > 1000 * bound, (gap, bound)                  # what lets the next assertion demand "all correct"
    v = verify.Verifier(final, "cuda")
    v.enroll_frames({sp: torch.from_numpy(xs.astype(F32)).cuda().contiguous() for sp, xs in enumerate(p["train"])}, col0=0)
    test = torch.from_numpy(np.concatenate([seg for _, seg in p["test"]]).astype(F32)).cuda().contiguous()
    segs = np.array([[50 * i, 50] for i in range(12)])
    sc = v.score_frames(test, segs, col0=0)
    assert sc.shape == (12, 3) and sc.dtype == np.float64
    llr = sc[:, 1:] - sc[:, :1]
    for i, (sp, seg) in enumerate(p["test"]):
        ref = [G.llr(seg, m, ubm) for m in ref_models]
        assert int(np.argmax(llr[i])) == sp, f"segment {i}: {llr[i]}"
        assert np.allclose(llr[i], ref, rtol=0, atol=1e-3 * gap)


# ------------------------------------------------------------------------------------------------------ audio end to end
def test_audio_end_to_end(tmp_path, capsys):
    from dvae_amd import evaluate as ev, verify
    corpus = G.voice_corpus()
    root, conv = tmp_path / "wav16", tmp_path / "converted"
    conv.mkdir()
    for name, wavs in corpus.items():
        (root / name).mkdir(parents=True)
        for i, w in enumerate(wavs):
            write_pcm16(root / name / f"{name}_{i:03d}.wav", w)
    held = [4, 5]
    for i in held:                                         # va's held-out files stand in for conversions to va
        write_pcm16(conv / f"convert_vb_to_va_{i:03d}.wav", corpus["va"][i])
    write_pcm16(conv / "convert_vb_to_va_silent.wav", np.zeros(16000, F32))
    ubm_path = tmp_path / "ubm.npz"
    assert verify.main(["train", str(root), "-o", str(ubm_path), "--components", "4", "--iters", "5"]) == 0
    train_out = capsys.readouterr().out
    lls = [float(v) for v in re.findall(r"^iteration \d+: mean log-likelihood (\S+)$", train_out, flags=re.M)]
    assert len(lls) == 5 and np.all(np.isfinite(lls))
    assert verify.main(["score", str(conv), "--ubm", str(ubm_path), "--target", str(root / "va"), "--source",
                        str(root / "vb"), "--enroll-utts", "4"]) == 0
    out = capsys.readouterr().out
    res = json.loads((conv / "verify.json").read_text())
    lines = dict((u, (float(a), float(b))) for u, a, b in
                 re.findall(r"^utterance (\S+) llr: target (\S+) source (\S+)$", out, flags=re.M))
    assert sorted(lines) == ["004", "005"] and "utterance silent llr: nan (no voiced frames)" in out
    assert "target accepted: 2/2" in out and "natural speech identified: 4/4" in out
    files = {r["utterance"]: r for r in res["files"]}
    for u, (a, b) in lines.items():
        assert (files[u]["llr_target"], files[u]["llr_source"], files[u]["accepted"]) == (a, b, True)
    assert files["silent"]["llr_target"] is None and files["silent"]["accepted"] is None
    assert res["no_voiced"] == [str(conv / "convert_vb_to_va_silent.wav")]
    assert (res["accepted"], res["scored"], res["components"], res["relevance"]) == (2, 2, 4, 16.0)
    assert res["natural"]["identified"] == 4 and res["natural"]["scored"] == 4 and res["ubm"] == str(ubm_path)
    mean_line = re.search(r"^mean llr: target (\S+) source (\S+) over 2 of 3 files$", out, flags=re.M)
    assert (float(mean_line.group(1)), float(mean_line.group(2))) == (res["mean_llr_target"], res["mean_llr_source"])
    assert res["mean_llr_target"] == np.mean([lines[u][0] for u in sorted(lines)])
    # the same decisions from gmm_ref in float64 on the GPU's own features
    ubm = verify.DiagGMM.load(ubm_path)
    um = (ubm.w, ubm.mu, ubm.var)
    fe = ev.MelCepstrum()
    wavs = [(np.clip(w, -1, 1) * 32767).astype("<i2").astype(F32) / 32768.0 for n in ("va", "vb") for w in corpus[n]]
    pk = fe.packed(wavs)
    feats = pk["feats"].cpu().numpy().astype(F64)
    per = [feats[r0:r0 + c, 1:24] for r0, c in zip(pk["table"][:, 0], pk["count"])]
    assert min(len(f) for f in per) > 100
    ta = G.tables(*um)
    ref_models = []
    for sp in range(2):
        xs = np.concatenate(per[6 * sp:6 * sp + 4])
        n, f, _ = G.stats(xs, G.loglik(xs, *ta)[2])
        ref_models.append(G.map_adapt(*um, n, f, len(xs)))
    segments = [(sp, per[6 * sp + i]) for sp in range(2) for i in held]
    gap, bound = margin_and_bound(segments, um, ref_models, 23)
    assert gap > 1000 * bound, (gap, bound)
    for u, i in (("004", 4), ("005", 5)):
        ref = [G.llr(per[i], m, um) for m in ref_models]
        assert np.allclose(lines[u], ref, rtol=0, atol=1e-3 * gap), (lines[u], ref)
    nat = {os.path.basename(r["file"]): r for r in res["natural"]["target"] + res["natural"]["source"]}
    for sp, name in enumerate(("va", "vb")):
        for i in held:
            r = nat[f"{name}_{i:03d}.wav"]
            ref = [G.llr(per[6 * sp + i], m, um) for m in ref_models]
            assert r["accepted"] is True and np.allclose([r["llr_target"], r["llr_source"]], ref, rtol=0, atol=1e-3 * gap)
