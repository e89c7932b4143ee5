"""The i-vector kernels of csrc/ivector.hip (dvae_gmm_utt_stats, dvae_ivec_posterior, dvae_ivec_accumulate; DESIGN.md section
4.21) on the MI355X through the C ABI, against the float64 restatement of tests/ivector_ref.py, and dvae_amd.ivector above
them.

The statistics are held to the summation bound against the float64 sums of the GPU's OWN gamma (from dvae_gmm_estep on the
same rows), the posterior to the backward and forward bounds of ivector_ref (operation counts and 2^-53, not what the kernel
gives), the accumulators to the summation bound against the GPU's own inputs, and what the contract calls bit-exact is
compared bit for bit: two calls, an utterance alone against the batch, null outputs, the all-zero utterance.  Every buffer a
launch may write is a guarded one of tests/kernel_harness.py, pre-filled with 0xFF.  The worst error / bound per shape is
printed at the module's end.
"""
import json
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, EINVAL, F32, F64, guards, ibuf, L, ok, Pad, st, Worst
import dvae_amd  # noqa: E402,F401
import gmm_ref as G  # noqa: E402
import ivector_ref as I  # noqa: E402
from test_hip_gmm import estep, make_frames, make_model, Tables  # noqa: E402
from test_ivector_ref import split  # noqa: E402
from test_mcd import write_pcm16  # noqa: E402

WORST = Worst("test_hip_ivector.py")
note = WORST.note
STAT_SHAPES = [(1, 1, 1, 0), (3, 23, 24, 1), (64, 23, 24, 1), (256, 32, 32, 0), (5, 7, 9, 2)]      # K, D, ldx, col0
COUNTS = [0, 1, 63, 64, 65, 300]
ACC_SHAPES = [(3, 5, 2), (5, 7, 17), (8, 3, 33)]                                                    # K, D, R


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def d64(a):
    return Buf(data=np.ascontiguousarray(a, F64))


# ---------------------------------------------------------------------------------------------------------- statistics
def utt_stats(xin, ldx, col0, segs, t):
    segs = np.ascontiguousarray(segs, np.int64).reshape(-1, 2)
    sb, n, f = ibuf(segs), Buf((len(segs), t.K), torch.float64), Buf((len(segs), t.K * t.D), torch.float64)
    ok(L().dvae_gmm_utt_stats(xin.ptr, ldx, col0, t.D, sb.ptr, len(segs), t.a.ptr, t.mu.ptr, t.prec.ptr, t.K, n.ptr, f.ptr,
                              st()), "dvae_gmm_utt_stats")
    guards(n, f, sb, xin.buf, t.a.buf, t.mu.buf, t.prec.buf)
    return n, f


@pytest.mark.parametrize("K,D,ldx,col0", STAT_SHAPES)
def test_utt_stats(K, D, ldx, col0):
    rs = np.random.RandomState(31 + K)
    model = make_model(rs, K, D)
    N = sum(COUNTS)
    x, full = make_frames(rs, N, model[1], model[2], ldx, col0)
    t = Tables([model])
    _, mu, prec = t.host[0]
    row0 = np.concatenate([[0], np.cumsum(COUNTS)[:-1]])
    segs = np.stack([row0, COUNTS], axis=1)                  # the segments tile the buffer
    _, gamma, stats, xin = estep(full, ldx, col0, N, t, want_lse=False)
    gg = gamma.np()
    n, f = utt_stats(xin, ldx, col0, segs, t)
    gn, gf = n.np(), f.np()
    n64, g64, an, ag = I.utt_sums(x, gg, segs)
    bn, bf = I.stats_bounds(COUNTS, an, ag, mu, prec)
    k = f"stats {K},{D},{ldx},{col0}"
    note((k, "n"), gn, n64, bn, "n")
    note((k, "f"), gf, I.centre_whiten(n64, g64, mu, prec), bf, "f")
    # the segments' n add up to the E-step's n over the same rows: two float64 sums of the same terms
    en = G.unpack_stats(stats.np(), K, D)[0]
    note((k, "sum n"), gn.sum(axis=0), en, 2 * G.sum_bound(N, an.sum(axis=0)) + G.sum_bound(len(segs), an.sum(axis=0)) + G.FLOOR,
         "sum_u n_uc against the E-step's n_c")
    assert not n.bits()[0].any() and not f.bits()[0].any(), "count = 0 writes +0.0 everywhere"
    for i in range(len(segs)):
        n1, f1 = utt_stats(xin, ldx, col0, segs[i:i + 1], t)
        assert np.array_equal(n1.bits()[0], n.bits()[i]) and np.array_equal(f1.bits()[0], f.bits()[i]), f"segment {i} alone"
    n2, f2 = utt_stats(xin, ldx, col0, segs, t)
    assert np.array_equal(n2.bits(), n.bits()) and np.array_equal(f2.bits(), f.bits())


# ----------------------------------------------------------------------------------------------------------- posterior
def run_posterior(n, f, T, P, want_S=True, want_ll=True):
    U, K, R = n.shape[0], n.shape[1], T.shape[1]
    D = T.shape[0] // K
    bufs = [d64(v) for v in (n, f, T, P)]
    w = Buf((U, R), torch.float64)
    S = Buf((U, R, R), torch.float64) if want_S else None
    ll = Buf((U,), torch.float64) if want_ll else None
    ok(L().dvae_ivec_posterior(*(b.ptr for b in bufs), U, K, D, R, w.ptr, S.ptr if S else None, ll.ptr if ll else None, st()),
       "dvae_ivec_posterior")
    guards(w, S, ll, *bufs)
    return w, S, ll


@pytest.mark.parametrize("U,K,D,R", I.POSTERIOR_SHAPES)
def test_posterior(U, K, D, R):
    n, f, T = I.posterior_inputs(U, K, D, R)
    P = I.gram(T, K, D)
    w, S, ll = run_posterior(n, f, T, P)
    gw, gS, gll = w.np(), S.np(), ll.np()
    assert np.isfinite(gw).all() and np.isfinite(gS).all() and np.isfinite(gll).all()
    ref = I.posterior_linalg(n, f, T, P)
    k = f"posterior {U},{K},{D},{R}"
    for u in range(U):
        rw, ri = I.backward_ratios(ref["L"][u], ref["b"][u], gw[u], gS[u], K, D, R)
        bw, bll, _ = I.forward_bounds(ref["L"][u], ref["w"][u], ref["ll"][u], K, D, R)
        bS = I.s_forward_bound(ref["L"][u], ref["w"][u], ref["inv"][u], K, D, R)
        for name, r in (("backward w", rw), ("backward inverse", ri),
                        ("forward w", np.linalg.norm(gw[u] - ref["w"][u]) / bw), ("forward ll", abs(gll[u] - ref["ll"][u]) / bll),
                        ("forward S", np.linalg.norm(gS[u] - ref["S"][u]) / bS),
                        ("symmetry", np.linalg.norm(gS[u] - gS[u].T) / (2.0 * bS))):
            WORST.record((k, name), float(r))
            assert r <= 1.0, f"{name}: utterance {u} of {(U, K, D, R)}: error / bound = {r:.3f}"
    if U >= 2:                                               # the all-zero utterance: exact, and +0.0
        assert not w.bits()[-1].any() and not ll.bits()[-1:].any()
        assert np.array_equal(S.bits()[-1], np.eye(R).view(np.int64))
    w2, S2, ll2 = run_posterior(n, f, T, P)
    assert np.array_equal(w2.bits(), w.bits()) and np.array_equal(S2.bits(), S.bits()) and np.array_equal(ll2.bits(), ll.bits())
    for want_S, want_ll in ((False, False), (True, False), (False, True)):
        w3, S3, ll3 = run_posterior(n, f, T, P, want_S, want_ll)
        assert np.array_equal(w3.bits(), w.bits()), "w does not depend on which optional outputs are asked for"
        assert S3 is None or np.array_equal(S3.bits(), S.bits())
        assert ll3 is None or np.array_equal(ll3.bits(), ll.bits())
    for u in sorted({0, min(1, U - 1), U - 1}):
        w1, S1, ll1 = run_posterior(n[u:u + 1], f[u:u + 1], T, P)
        assert np.array_equal(w1.bits()[0], w.bits()[u]) and np.array_equal(S1.bits()[0], S.bits()[u])
        assert np.array_equal(ll1.bits()[0], ll.bits()[u]), f"utterance {u}: alone and in the batch"


def test_posterior_nonfinite_input_stays_in_its_utterance():
    U, K, D, R = 7, 4, 5, 3
    n, f, T = I.posterior_inputs(U, K, D, R)
    P = I.gram(T, K, D)
    w, S, ll = run_posterior(n, f, T, P)
    f2, n2 = f.copy(), n.copy()
    f2[2, 1], n2[4, 0] = np.nan, np.inf
    wb, Sb, llb = run_posterior(n2, f2, T, P)
    for u in range(U):
        if u in (2, 4):
            assert np.isnan(wb.np()[u]).all() and np.isnan(llb.np()[u])
        else:
            assert np.array_equal(wb.bits()[u], w.bits()[u]) and np.array_equal(Sb.bits()[u], S.bits()[u])
            assert np.array_equal(llb.bits()[u], ll.bits()[u])


# ---------------------------------------------------------------------------------------------------------- accumulate
def ws_buf(U, K, D, R):
    need = L().dvae_ivec_ws_bytes(U, K, D, R)
    assert need > 0 and need % 8 == 0
    b = Buf((need + 512,), torch.uint8)
    b.slack_from = need
    return b, need


def run_accumulate(n, f, w, S):
    U, K, R = n.shape[0], n.shape[1], w.shape[1]
    D = f.shape[1] // K
    bufs = [d64(v) for v in (n, f, w, S)]
    ws, _ = ws_buf(U, K, D, R)
    A, C, Ss = Buf((K, R, R), torch.float64), Buf((K * D, R), torch.float64), Buf((R, R), torch.float64)
    ok(L().dvae_ivec_accumulate(*(b.ptr for b in bufs), U, K, D, R, ws.ptr, A.ptr, C.ptr, Ss.ptr, st()), "dvae_ivec_accumulate")
    guards(ws, A, C, Ss, *bufs)
    return A, C, Ss


@pytest.mark.parametrize("U", [1, 2, 65, 257])
@pytest.mark.parametrize("K,D,R", ACC_SHAPES)
def test_accumulate(K, D, R, U):
    rs = np.random.RandomState(100 * U + R)
    n, f = rs.uniform(0.0, 50.0, (U, K)), rs.randn(U, K * D) * 5.0
    w, S = rs.randn(U, R), rs.randn(U, R, R)
    A, C, Ss = run_accumulate(n, f, w, S)
    rA, rC, rS = I.accumulators(n, f, w, S)
    aA, aC, aS = I.accumulators_abs(n, f, w, S)
    k = f"accumulate {K},{D},{R}"
    note((k, "A"), A.np(), rA, I.sum_bound(U, aA) + G.FLOOR, f"A U={U}")
    note((k, "C"), C.np(), rC, I.sum_bound(U, aC) + G.FLOOR, f"C U={U}")
    note((k, "Ssum"), Ss.np(), rS, I.sum_bound(U, aS) + G.FLOOR, f"Ssum U={U}")
    A2, C2, S2 = run_accumulate(n, f, w, S)
    assert np.array_equal(A2.bits(), A.bits()) and np.array_equal(C2.bits(), C.bits()) and np.array_equal(S2.bits(), Ss.bits())
    groups = -(-U // max(64, -(-U // 8)))                      # groups of max(64, ceil(U / 8)) utterances
    assert ws_buf(U, K, D, R)[1] == groups * (K * R * R + K * D * R + R * R) * 8
    if U == 1:                                               # one term: exact
        assert np.array_equal(A.np(), n[0][:, None, None] * S[0][None]) and np.array_equal(Ss.np(), S[0])


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing():
    K, D, ldx, col0, N = 5, 7, 9, 2, 40
    rs = np.random.RandomState(3)
    model = make_model(rs, K, D)
    _, full = make_frames(rs, N, model[1], model[2], ldx, col0)
    t, xin = Tables([model]), Pad(full)
    big = Pad(np.zeros((257, 33), F32))
    segs = ibuf(np.array([[0, N]], np.int64))

    def refused(rc, *outs):
        assert rc == EINVAL, rc
        guards(*outs)
        for b in outs:
            assert b.poisoned().all(), "a refused call wrote an output"

    def s(x=xin.ptr, ldx=ldx, col0=col0, D=D, sg=segs.ptr, nseg=1, a=t.a.ptr, mu=t.mu.ptr, prec=t.prec.ptr, K=K, n=0, f=0):
        nb, fb = Buf((4, 8), torch.float64), Buf((4, 64), torch.float64)
        refused(L().dvae_gmm_utt_stats(x, ldx, col0, D, sg, nseg, a, mu, prec, K, None if n is None else nb.ptr + n,
                                       None if f is None else fb.ptr + f, st()), nb, fb)

    for kw in (dict(x=None), dict(sg=None), dict(a=None), dict(mu=None), dict(prec=None), dict(n=None), dict(f=None),
               dict(nseg=0), dict(K=0), dict(D=0), dict(K=257, a=big.ptr, mu=big.ptr, prec=big.ptr),
               dict(D=33, ldx=40, mu=big.ptr, prec=big.ptr), dict(col0=-1), dict(ldx=col0 + D - 1), dict(n=4), dict(f=4),
               dict(sg=segs.ptr + 4)):
        s(**kw)

    U, K, D, R = 3, 4, 5, 3
    n, f, T = I.posterior_inputs(U, K, D, R)
    ins = {k: d64(v) for k, v in dict(n=n, f=f, T=T, P=I.gram(T, K, D)).items()}
    wide = d64(np.zeros(257 * 33 * 65))

    def p(U=U, K=K, D=D, R=R, w=0, S=0, ll=0, **over):
        a = {k: b.ptr for k, b in ins.items()}
        a.update(over)
        wb, Sb, lb = Buf((4, 66), torch.float64), Buf((4, 66), torch.float64), Buf((8,), torch.float64)
        refused(L().dvae_ivec_posterior(a["n"], a["f"], a["T"], a["P"], U, K, D, R, None if w is None else wb.ptr + w,
                                        Sb.ptr + S, lb.ptr + ll, st()), wb, Sb, lb)

    for kw in (dict(n=None), dict(f=None), dict(T=None), dict(P=None), dict(w=None), dict(U=0), dict(K=0), dict(D=0),
               dict(R=0), dict(U=-1), dict(R=65, T=wide.ptr, P=wide.ptr), dict(K=257, n=wide.ptr, f=wide.ptr, T=wide.ptr, P=wide.ptr),
               dict(D=33, f=wide.ptr, T=wide.ptr), dict(w=4), dict(S=4), dict(ll=4), dict(n=ins["n"].ptr + 4),
               dict(P=ins["P"].ptr + 4)):
        p(**kw)

    acc = {k: d64(v) for k, v in dict(n=n, f=f, w=np.zeros((U, R)), S=np.zeros((U, R, R))).items()}

    def a_(U=U, K=K, D=D, R=R, ws=0, A=0, C=0, Ss=0, **over):
        a = {k: b.ptr for k, b in acc.items()}
        a.update(over)
        wsb, Ab, Cb, Sb = Buf((1 << 14,), torch.uint8), Buf((64,), torch.float64), Buf((64,), torch.float64), Buf((16,), torch.float64)
        refused(L().dvae_ivec_accumulate(a["n"], a["f"], a["w"], a["S"], U, K, D, R, None if ws is None else wsb.ptr + ws,
                                         None if A is None else Ab.ptr + A, None if C is None else Cb.ptr + C,
                                         None if Ss is None else Sb.ptr + Ss, st()), wsb, Ab, Cb, Sb)

    for kw in (dict(n=None), dict(f=None), dict(w=None), dict(S=None), dict(ws=None), dict(A=None), dict(C=None), dict(Ss=None),
               dict(U=0), dict(K=0), dict(D=0), dict(R=0), dict(R=65), dict(K=257), dict(D=33), dict(ws=4), dict(A=4),
               dict(C=4), dict(Ss=4), dict(S=acc["S"].ptr + 4)):
        a_(**kw)
    W = L().dvae_ivec_ws_bytes
    assert W(0, K, D, R) == 0 and W(U, 0, D, R) == 0 and W(U, K, 0, R) == 0 and W(U, K, D, 0) == 0
    assert W(U, 257, D, R) == 0 and W(U, K, 33, R) == 0 and W(U, K, D, 65) == 0 and W(U, K, D, 64) > 0


# ------------------------------------------------------------------------------------ the trainer and the planted speakers
@pytest.fixture(scope="module")
def planted_gpu():
    """the planted utterances' statistics from dvae_gmm_utt_stats, as the package forms them"""
    from dvae_amd import ivector, verify
    p = I.planted()
    ubm = verify.DiagGMM(*p["ubm"])
    feats = torch.from_numpy(p["x"].astype(F32)).cuda().contiguous()
    n, f = ivector.utterance_stats(feats, p["segs"], ubm, col0=0)
    return p, ubm, feats, n, f


def test_one_em_step_does_not_drift(planted_gpu):
    from dvae_amd import ivector
    p, ubm, feats, n, f = planted_gpu
    K, D, R = p["K"], p["D"], p["R"]
    tr = torch.from_numpy(np.nonzero(split(p))[0]).cuda()
    nt, ft = n[tr].contiguous(), f[tr].contiguous()
    n64, f64, U = nt.cpu().numpy(), ft.cpu().numpy(), int(nt.shape[0])
    for min_div in (True, False):
        hist = []
        final, lls = ivector.train_extractor(nt, ft, R, iters=5, seed=0, min_divergence=min_div, batch=16, history=hist)
        assert len(hist) == 5 and len(lls) == 5 and np.array_equal(hist[0]["T"], I.init_T(K, D, R, 0))
        Ts = [h["T"] for h in hist] + [final]
        for i in range(4):
            T_ref, ll_ref, post = I.em_step(n64, f64, Ts[i], K, D, min_div, post=I.posterior_linalg)
            note(("em step", f"T min_div={min_div}"), Ts[i + 1], T_ref, I.em_step_bound(n64, f64, Ts[i], K, D, min_div),
                 f"T after iteration {i}")
            bll = sum(I.forward_bounds(post["L"][u], post["w"][u], post["ll"][u], K, D, R)[1] for u in range(U))
            note(("em step", "sum ll"), [hist[i]["ll"]], [ll_ref], [bll + I.sum_bound(U, np.abs(post["ll"]).sum())], f"ll {i}")
            assert hist[i + 1]["ll"] >= hist[i]["ll"] - 2.0 * bll, "the bound falls by more than its rounding"
        # chunks of 16 against one chunk: other partial sums of the same terms
        one, lls1 = ivector.train_extractor(nt, ft, R, iters=1, seed=0, min_divergence=min_div, batch=4096)
        assert np.allclose(one, Ts[1], rtol=0, atol=2 * I.em_step_bound(n64, f64, Ts[0], K, D, min_div).max())
        again, lls2 = ivector.train_extractor(nt, ft, R, iters=5, seed=0, min_divergence=min_div, batch=16)
        assert np.array_equal(again, final) and lls2 == lls, "two trainings give the same bits"


def test_planted_speakers_end_to_end(planted_gpu):
    from dvae_amd import ivector
    p, ubm, feats, n, f = planted_gpu
    K, D, R = p["K"], p["D"], p["R"]
    trm, spk = split(p), p["speaker"]
    tr = torch.from_numpy(np.nonzero(trm)[0]).cuda()
    T, lls = ivector.train_extractor(n[tr].contiguous(), f[tr].contiguous(), R, iters=8, seed=0)
    assert np.all(np.diff(lls) > -1e-9)
    # the float64 pipeline from the GPU's T and statistics: a margin no rounding turns
    n64, f64, P = n.cpu().numpy(), f.cpu().numpy(), I.gram(T, K, D)
    post = I.posterior_linalg(n64, f64, T, P)
    cos64, mean, W = I.identify(post["w"][trm], spk[trm], post["w"][~trm])
    gap = I.margin(cos64, spk[~trm])
    dw = max(I.forward_bounds(post["L"][u], post["w"][u], post["ll"][u], K, D, R)[0] for u in range(len(n64)))
    bound = I.cosine_bound(dw, post["w"], mean, W)
    assert gap > 100 * bound, (gap, bound)
    ex = ivector.Extractor(ubm, T)
    w = ex.extract_frames(feats, p["segs"], col0=0)
    assert w.shape == (48, R) and w.dtype == np.float64
    for u in range(48):
        note(("end to end", "w"), [np.linalg.norm(w[u] - post["w"][u])], [0.0],
             [I.forward_bounds(post["L"][u], post["w"][u], post["ll"][u], K, D, R)[0]], f"i-vector {u}")
    ex.backend = ivector.Backend.fit(w[trm])
    y = ex.backend.transform(w)
    models = np.stack([ivector.Backend.speaker(y[trm & (spk == s)]) for s in range(6)])
    cos = ivector.cosine_scores(y[~trm], models)
    assert np.array_equal(np.argmax(cos, axis=1), spk[~trm]), cos
    assert np.allclose(cos, cos64, rtol=0, atol=1e-3 * gap)
    segs0 = np.concatenate([p["segs"][:2], [[5, 0]]])
    w0 = ex.extract_frames(feats, segs0, col0=0)
    assert np.isnan(w0[2]).all() and np.array_equal(w0[:2], w[:2]), "no frames: a NaN row; the others keep their bits"


# ------------------------------------------------------------------------------------------------------ audio end to end
def test_audio_end_to_end(tmp_path, capsys):
    from dvae_amd import ivector, verify
    corpus = G.voice_corpus()
    root, conv = tmp_path / "wav16", tmp_path / "converted"
    conv.mkdir()
    for name, wavs in corpus.items():
        (root / name).mkdir(parents=True)
        for i, wv in enumerate(wavs):
            write_pcm16(root / name / f"{name}_{i:03d}.wav", wv)
    held = [4, 5]
    for i in held:                                         # va's held-out files stand in for conversions to va
        write_pcm16(conv / f"convert_vb_to_va_{i:03d}.wav", corpus["va"][i])
    write_pcm16(conv / "convert_vb_to_va_silent.wav", np.zeros(16000, F32))
    ubm_path, iv_path, iv2_path = tmp_path / "ubm.npz", tmp_path / "ivec.npz", tmp_path / "ivec2.npz"
    # ONE component: an i-vector lives in the first-order statistics around components that the speakers SHARE.  Each voice
    # here is two tight clusters (its two F0 values: the harmonics are resolved in the cepstra), and a mixture with a
    # component per cluster leaves nothing but noise around its means
    assert verify.main(["train", str(root), "-o", str(ubm_path), "--components", "1", "--iters", "3"]) == 0
    capsys.readouterr()
    train_args = ["train", str(root), "--ubm", str(ubm_path), "--rank", "2", "--iters", "5"]
    assert ivector.main(train_args + ["-o", str(iv_path)]) == 0
    out = capsys.readouterr().out
    assert "2 speakers, 12 utterances (0 without voiced frames left out)" in out and f"wrote {iv_path}" in out
    lls = [float(v) for v in re.findall(r"^iteration \d+: mean log-likelihood bound (\S+)$", out, flags=re.M)]
    assert len(lls) == 5 and np.all(np.isfinite(lls)) and np.all(np.diff(lls) > -1e-9 * np.abs(lls[:-1]))
    assert ivector.main(train_args + ["-o", str(iv2_path)]) == 0
    capsys.readouterr()
    with np.load(iv_path) as z1, np.load(iv2_path) as z2:
        assert sorted(z1.files) == sorted(z2.files) and {"T", "ubm_mu", "backend_W", "config_batch"} <= set(z1.files)
        for k in z1.files:
            assert z1[k].tobytes() == z2[k].tobytes(), f"{k}: two trainings differ"
        assert z1["config_batch"].item() == 4096 and z1["config_rank"].item() == 2 and z1["T"].shape == (1 * 23, 2)
    # score
    assert ivector.main(["score", str(conv), "--ubm", str(ubm_path), "--ivector", str(iv_path), "--target", str(root / "va"),
                         "--source", str(root / "vb"), "--enroll-utts", "4"]) == 0
    out = capsys.readouterr().out
    res = json.loads((conv / "ivector.json").read_text())
    lines = dict((u, (float(a), float(b))) for u, a, b in
                 re.findall(r"^utterance (\S+) cos: target (\S+) source (\S+)$", out, flags=re.M))
    assert sorted(lines) == ["004", "005"] and "utterance silent cos: nan (no voiced frames)" in out
    assert "target accepted: 2/2" in out and "natural speech identified: 4/4" in out
    files = {r["utterance"]: r for r in res["files"]}
    for u, (a, b) in lines.items():
        assert (files[u]["cos_target"], files[u]["cos_source"], files[u]["accepted"]) == (a, b, True)
        assert a > b and -1.0 - 1e-12 <= b and a <= 1.0 + 1e-12
    assert files["silent"]["cos_target"] is None and files["silent"]["accepted"] is None
    assert res["no_voiced"] == [str(conv / "convert_vb_to_va_silent.wav")]
    assert (res["accepted"], res["scored"], res["components"], res["rank"], res["enroll_utts"]) == (2, 2, 1, 2, 4)
    assert res["natural"]["identified"] == 4 and res["natural"]["scored"] == 4 and res["ivector"] == str(iv_path)
    assert all(r["accepted"] is True for r in res["natural"]["target"] + res["natural"]["source"])
    mean_line = re.search(r"^mean cos: target (\S+) source (\S+) over 2 of 3 files$", out, flags=re.M)
    assert (float(mean_line.group(1)), float(mean_line.group(2))) == (res["mean_cos_target"], res["mean_cos_source"])
    assert res["mean_cos_target"] == np.mean([lines[u][0] for u in sorted(lines)])
    # eer: both instruments on the same trials, with a silent file among them
    write_pcm16(root / "vb" / "vb_999.wav", np.zeros(16000, F32))
    ej = tmp_path / "eer.json"
    assert ivector.main(["eer", str(root), "--ubm", str(ubm_path), "--ivector", str(iv_path), "--enroll-utts", "4",
                         "--json", str(ej)]) == 0
    out = capsys.readouterr().out
    m = re.search(r"^eer cosine: (\S+) % \((\d+) target, (\d+) non-target trials\)$", out, flags=re.M)
    m2 = re.search(r"^eer llr: (\S+) % \((\d+) target, (\d+) non-target trials\)$", out, flags=re.M)
    assert m and m2 and float(m.group(1)) == 0.0 and (m.group(2), m.group(3)) == ("4", "4") == (m2.group(2), m2.group(3))
    assert 0.0 <= float(m2.group(1)) <= 100.0
    assert f"no voiced frames: {root / 'vb' / 'vb_999.wav'}" in out
    rj = json.loads(ej.read_text())
    assert rj["cosine"]["eer_percent"] == float(m.group(1)) and rj["llr"]["eer_percent"] == float(m2.group(1))
    assert rj["no_voiced"] == [str(root / "vb" / "vb_999.wav")] and rj["speakers"] == ["va", "vb"]
    # a UBM other than the extractor's own is refused
    other = tmp_path / "other.npz"
    assert verify.main(["train", str(root), "-o", str(other), "--components", "3", "--iters", "2"]) == 0
    with pytest.raises(ValueError, match="another UBM"):
        ivector.main(["eer", str(root), "--ubm", str(other), "--ivector", str(iv_path), "--enroll-utts", "4"])
