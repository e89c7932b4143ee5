"""Whole-utterance conversion on the MI355X: the three window kernels of csrc/elem.hip through the C ABI against the float64
restatement of tests/convert_ref.py, the engine (dvae_amd.convert.Converter) against the same model calls and launches
composed by hand, and the wav-to-wav command in a child process.

Every launch writes into guarded buffers of tests/kernel_harness.py filled with 0xFF; the packed mels hold NaN in the columns
that no utterance owns.  What the restatement derives as bits (the copies, one covering window, the style at mix 0 and 1) is
compared bit for bit, the rest within its derived bound at every element.  Worst error / bound measured on an MI355X:
overlap_add 0.972, window_latents at mix 0.37 0.799 — the bound is little more than the store's one rounding to fp32
(2^-24 of the value), and a value just above a power of two uses nearly all of it.
"""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import (assert_same_bits, Buf, dev_equal, EINVAL, F32, F64, guards, ibuf, L, make_trainer, ok, ROOT, st,  # noqa: E402
                            untouched, Worst)
import dvae_amd  # noqa: E402,F401
import convert_ref as R  # noqa: E402

WORST = Worst("test_hip_convert.py", sort=True)
note = WORST.note
I32 = np.int32


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def _tables(d):
    return ibuf(d["utt"], I32), ibuf(d["win"], I32)


# ------------------------------------------------------------------------------------------------------- mel_to_windows
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_mel_to_windows(c):
    d = R.case_data(c)
    utt, win = _tables(d)
    mels = Buf(data=d["mels"])
    n = len(d["win"])
    out = Buf((n, c["C"], c["T"]))
    ok(L().dvae_mel_to_windows(mels.ptr, d["ld"], utt.ptr, win.ptr, out.ptr, n, c["C"], c["T"], st()))
    guards(out, mels, utt, win)
    got = out.np()
    assert np.isfinite(got).all(), "a column no utterance owns (NaN) was read into a window, or an element was not written"
    assert_same_bits(out, R.mel_to_windows(d["mels"], d["utt"], d["win"], c["T"]), "mel_to_windows")
    assert not out.bits()[d["nwin"]:].any(), "a padding window is +0.0 throughout"


def test_mel_to_windows_einval():
    c = R.CASES[0]
    d = R.case_data(c)
    utt, win = _tables(d)
    mels, n = Buf(data=d["mels"]), len(d["win"])
    out = Buf((n, c["C"], c["T"]))
    good = [mels.ptr, d["ld"], utt.ptr, win.ptr, out.ptr, n, c["C"], c["T"]]
    for i, bad in ((0, None), (2, None), (3, None), (4, None), (1, 0), (5, 0), (6, 0), (7, 0), (5, -1)):
        a = list(good)
        a[i] = bad
        assert L().dvae_mel_to_windows(*a, st()) == EINVAL, i
    untouched(out.bits(), "mel_to_windows after EINVAL")


# ------------------------------------------------------------------------------------------------------- window_latents
@pytest.mark.parametrize("mix", [0.0, 1.0, 0.37])
def test_window_latents(mix):
    c = R.latent_case()
    S, Cn, n = c["S"], c["Cn"], len(c["g_src"])
    content, sums, counts = Buf(data=c["content"]), Buf(data=c["sums"]), Buf(data=c["counts"])
    gs, gt = ibuf(c["g_src"], I32), ibuf(c["g_trg"], I32)
    z = Buf((n, S + Cn))
    args = (content.ptr, sums.ptr, counts.ptr, gs.ptr, gt.ptr, mix, z.ptr, n, S, Cn, 2 * S)
    ok(L().dvae_window_latents(*args, st()))
    guards(z)
    first = z.bits()
    ref, tol = R.window_latents(c["content"], c["sums"], c["counts"], c["g_src"], c["g_trg"], mix, S)
    got = z.np()
    assert_same_bits(got[:-1, S:], c["content"][:-1, :Cn], "content columns are copies")
    assert not first[-1].any(), "a padding row is +0.0"
    if mix in (0.0, 1.0):
        assert_same_bits(got[:, :S], ref[:, :S].astype(F32), f"style at mix {mix}")
    else:
        assert (tol[:-1, :S] > 0).all() and (tol[:-1, :S] <= np.spacing(np.abs(ref[:-1, :S]).astype(F32)) + 2.0 ** -125).all()
        note(f"window_latents mix {mix}", got[:-1, :S], ref[:-1, :S], tol[:-1, :S], "style columns")
    assert R.latents_close(got, ref, tol)
    z2 = Buf((n, S + Cn))
    ok(L().dvae_window_latents(*args[:6], z2.ptr, *args[7:], st()))
    assert np.array_equal(first, z2.bits()), "a second launch gives the same bits"


def test_window_latents_einval_and_the_empty_group():
    c = R.latent_case()
    S, Cn, n = c["S"], c["Cn"], len(c["g_src"])
    content, sums, counts = Buf(data=c["content"]), Buf(data=c["sums"]), Buf(data=c["counts"])
    gs, gt = ibuf(c["g_src"], I32), ibuf(c["g_trg"], I32)
    z = Buf((n, S + Cn))
    good = [content.ptr, sums.ptr, counts.ptr, gs.ptr, gt.ptr, 1.0, z.ptr, n, S, Cn, 2 * S]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (6, None), (7, 0), (8, 0), (9, 0), (10, S - 1),
                   (5, -0.1), (5, 1.5), (5, float("nan"))):
        a = list(good)
        a[i] = bad
        assert L().dvae_window_latents(*a, st()) == EINVAL, i
    untouched(z.bits(), "window_latents after EINVAL")
    # an empty group in use: refused on the host side, before any launch
    from dvae_amd import convert
    from dvae_amd._lib import DvaeHipError
    empty = c["counts"].copy()
    empty[1] = 0
    with pytest.raises(DvaeHipError, match="rc=-1"):
        convert.window_latents(content.t, sums.t, counts.t, gs.t, gt.t, 1.0, S, counts_host=empty)
    zt = convert.window_latents(content.t, sums.t, counts.t, gs.t, gt.t, 1.0, S, counts_host=c["counts"])
    assert_same_bits(zt.cpu().numpy(), R.window_latents(c["content"], c["sums"], c["counts"], c["g_src"], c["g_trg"], 1.0, S)[0]
                     .astype(F32), "the wrapper's launch")


# -------------------------------------------------------------------------------------------------- windows_overlap_add
def _ola(d, c, y, clamp=None):
    utt, win = _tables(d)
    yb, wb = Buf(data=y), Buf(data=d["w32"])
    out = Buf((c["C"], d["ld"]))
    lo, hi = clamp or (0.0, 0.0)
    ok(L().dvae_windows_overlap_add(yb.ptr, utt.ptr, win.ptr, wb.ptr, out.ptr, d["ld"], len(d["utt"]), c["C"], c["T"], lo, hi,
                                    int(clamp is not None), st()))
    guards(out, yb, wb, utt, win)
    return out


def _hold(out, res, what):
    got, o, s = out.np(), res["owned"], res["single"]
    untouched(out.bits()[~o], what + ": columns between utterances")
    assert np.isfinite(got[o]).all(), what + ": an owned element was not written"
    assert_same_bits(got[s], res["ref"][s].astype(F32), what + ": one window covers, bits")
    m = o & ~s
    if m.any():
        note("overlap_add", got[m], res["ref"][m], res["tol"][m], what)
    assert R.close(got, res)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_windows_overlap_add(c):
    d = R.case_data(c)
    out = _ola(d, c, d["y"])
    _hold(out, R.overlap_add(d["y"], d["utt"], d["win"], d["w32"], d["ld"]), "overlap_add")
    assert np.array_equal(out.bits(), _ola(d, c, d["y"]).bits()), "a second launch gives the same bits"
    # the clamp: the stand-ins reach from -0.2 to 1.2
    res = R.overlap_add(d["y"], d["utt"], d["win"], d["w32"], d["ld"], clamp=(0.0, 1.0))
    got = _ola(d, c, d["y"], clamp=(0.0, 1.0))
    _hold(got, res, "overlap_add clamped")
    v = got.np()[res["owned"]]
    assert v.min() >= 0.0 and v.max() <= 1.0


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_cut_and_overlap_add_is_the_identity_on_the_device(c):
    d = R.case_data(c)
    utt, win = _tables(d)
    mels, n = Buf(data=d["mels"]), len(d["win"])
    wins = Buf((n, c["C"], c["T"]))
    ok(L().dvae_mel_to_windows(mels.ptr, d["ld"], utt.ptr, win.ptr, wins.ptr, n, c["C"], c["T"], st()))
    out = _ola(d, c, wins.np())
    res = R.overlap_add(wins.np(), d["utt"], d["win"], d["w32"], d["ld"])
    _hold(out, res, "identity")
    X, o, s = d["mels"], res["owned"], res["single"]
    got = out.np()
    assert_same_bits(got[s], X[s], "identity: bits where one window covers")
    assert (np.abs(got[o].astype(F64) - X[o].astype(F64)) <= np.maximum(res["tol"][o], 0)).all(), "identity within the bound"


def test_windows_overlap_add_einval():
    c = R.CASES[0]
    d = R.case_data(c)
    utt, win = _tables(d)
    yb, wb, out = Buf(data=d["y"]), Buf(data=d["w32"]), Buf((c["C"], d["ld"]))
    good = [yb.ptr, utt.ptr, win.ptr, wb.ptr, out.ptr, d["ld"], len(d["utt"]), c["C"], c["T"], 0.0, 1.0, 1]
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, 0), (7, 0), (8, 0), (6, -2)):
        a = list(good)
        a[i] = bad
        assert L().dvae_windows_overlap_add(*a, st()) == EINVAL, i
    a = list(good)
    a[9], a[10] = 1.0, 0.0
    assert L().dvae_windows_overlap_add(*a, st()) == EINVAL, "lo > hi"
    untouched(out.bits(), "windows_overlap_add after EINVAL")


# --------------------------------------------------------------------------------------------------------------- engine
T, BATCH, LENGTHS = 64, 4, (150, 64, 40)


@pytest.fixture(scope="module")
def engine():
    from dvae_amd import convert
    tr = make_trainer(batch=BATCH, n_frames=T)
    rs = np.random.RandomState(7)
    sources = [rs.rand(80, n).astype(F32) for n in LENGTHS]
    targets = {"a": [rs.rand(80, 100).astype(F32), rs.rand(80, 70).astype(F32)], "b": [rs.rand(80, 64).astype(F32)]}
    conv = convert.Converter(tr, batch=BATCH, checkpoint="DisentangledVAE_VCTK_1.pth")
    assert conv.hop == T // 2
    bank = conv.style_bank(targets)
    res = conv.convert(sources, ["a", "b", "a"], bank, style_mix=0.6, recons=True)
    torch.cuda.synchronize()
    return dict(tr=tr, conv=conv, sources=sources, targets=targets, bank=bank, res=res, convert=convert)


def _by_hand(tr, sources, sums_bank, counts_bank, trg, mix, hop, batch):
    """The engine's sequence of model calls and launches, composed from the C ABI and the model alone."""
    from dvae_amd import ops
    m, lib, dev = tr.model, L(), "cuda"
    S, Cn = m.speaker_size, m.latent_dim - m.speaker_size
    utt, win, ld, _ = R.plan([s.shape[1] for s in sources], T, hop, batch)
    n, nutt = len(win), len(utt)
    packed = torch.zeros((80, ld), device=dev)
    for s, (col0, n_fr, _, _) in zip(sources, utt):
        packed[:, col0:col0 + n_fr] = torch.from_numpy(s).to(dev)
    utt_d, win_d = torch.from_numpy(utt.astype(I32)).to(dev), torch.from_numpy(win.astype(I32)).to(dev)
    w = torch.from_numpy(R.window(T).astype(F32)).to(dev)
    was = m.training
    m.eval()
    try:
        with torch.no_grad():
            x = torch.empty((n, 80, T), device=dev)
            ok(lib.dvae_mel_to_windows(packed.data_ptr(), ld, utt_d.data_ptr(), win_d.data_ptr(), x.data_ptr(), n, 80, T, st()))
            heads = [m.encode_heads(x[a:a + batch]) for a in range(0, n, batch)]
            style = torch.cat([h[0].clone() for h in heads]).contiguous()
            content = torch.cat([h[1].clone() for h in heads]).contiguous()
            g_src = win_d[:, 0].contiguous()
            sums = torch.zeros((nutt + 1, 2 * S), dtype=torch.float64, device=dev)
            cnt = torch.zeros(2 * (nutt + 1), dtype=torch.int64, device=dev)
            ops.group_sum(style, g_src, sums, cnt[:nutt + 1], cnt[nutt + 1:])
            sums = torch.cat([sums[:nutt], torch.from_numpy(sums_bank).to(dev)]).contiguous()
            cnt = torch.cat([cnt[:nutt], torch.from_numpy(counts_bank).to(dev)]).contiguous()
            u = win[:, 0]
            g_trg = torch.from_numpy(np.where(u >= 0, nutt + np.asarray(trg)[np.maximum(u, 0)], -1).astype(I32)).to(dev)

            def latents(gt, mx):
                z = torch.empty((n, S + Cn), device=dev)
                ok(lib.dvae_window_latents(content.data_ptr(), sums.data_ptr(), cnt.data_ptr(), g_src.data_ptr(), gt.data_ptr(),
                                           mx, z.data_ptr(), n, S, Cn, 2 * S, st()))
                return z

            def decode(z, post):
                ys = []
                for a in range(0, n, batch):
                    d_ = m.decode(z[a:a + batch])
                    ys.append((m.postnet.forward_plus_input(d_) if post else d_).clone())
                return torch.cat(ys).contiguous()

            def ola(y, clamp):
                out = torch.empty((80, ld), device=dev)
                ok(lib.dvae_windows_overlap_add(y.data_ptr(), utt_d.data_ptr(), win_d.data_ptr(), w.data_ptr(), out.data_ptr(),
                                                ld, nutt, 80, T, 0.0, 1.0 if clamp else 0.0, int(clamp), st()))
                return out

            conv = ola(decode(latents(g_trg, mix), True), True)
            rec = ola(decode(latents(g_src, 0.0), False), False)
    finally:
        m.train(was)
    cut = lambda o: [o[:, col0:col0 + n_fr].contiguous() for col0, n_fr, _, _ in utt]
    return cut(conv), cut(rec)


def test_engine_shapes_and_hand_composition(engine):
    e = engine
    assert e["tr"].model.training, "convert leaves model.training as it found it"
    for r, n in zip(e["res"], LENGTHS):
        assert sorted(r) == ["converted", "decoded", "recons"]
        assert all(tuple(v.shape) == (80, n) and v.dtype == torch.float32 for v in r.values()), "exactly L frames"
        assert bool(torch.isfinite(r["converted"]).all()) and float(r["converted"].min()) >= 0.0 and float(r["converted"].max()) <= 1.0
    conv, rec = _by_hand(e["tr"], e["sources"], e["bank"].sums, e["bank"].counts, [0, 1, 0], 0.6, T // 2, BATCH)
    for r, c_, r_ in zip(e["res"], conv, rec):
        assert dev_equal(r["converted"], c_), "converted: the hand-composed launches give other bits"
        assert dev_equal(r["recons"], r_), "recons: the hand-composed launches give other bits"
    assert e["bank"].names == ["a", "b"] and e["bank"].counts.tolist() == [3 + 2, 1] and e["bank"].sums.shape == (2, 8)
    assert (e["bank"].T, e["bank"].hop, e["bank"].S, e["bank"].checkpoint) == (T, T // 2, 4, "DisentangledVAE_VCTK_1.pth")


def test_engine_second_call_and_saved_bank_give_the_same_bits(engine, tmp_path):
    e = engine
    again = e["conv"].convert(e["sources"], ["a", "b", "a"], e["bank"], style_mix=0.6, recons=True)
    path = e["bank"].save(tmp_path / "bank.npz")
    loaded = e["conv"].convert(e["sources"], ["a", "b", "a"], e["convert"].StyleBank.load(path), style_mix=0.6, recons=True)
    for r, a, b in zip(e["res"], again, loaded):
        for k in r:
            assert dev_equal(r[k], a[k]), f"{k}: a second call gives other bits"
            assert dev_equal(r[k], b[k]), f"{k}: a saved and loaded bank gives other bits"
    # the delegate of the trainer: the same engine
    via = e["tr"].convert_utterances(e["sources"], ["a", "b", "a"], e["bank"], style_mix=0.6, batch=BATCH)
    assert all(dev_equal(r["converted"], v["converted"]) for r, v in zip(e["res"], via)) and e["tr"].model.training


def test_engine_style_mix_zero_is_the_reconstruction(engine):
    e = engine
    own = e["conv"].style_bank({"self": [e["sources"][0]]})
    r = e["conv"].convert(e["sources"][:1], "self", own, style_mix=0.0, recons=True)[0]
    assert dev_equal(r["decoded"], r["recons"]), "mix 0: the converted path before the post-net is the reconstruction"
    # and with the source as its own target group the mix does not matter: the same windows in the same rows, the same sums
    r1 = e["conv"].convert(e["sources"][:1], "self", own, style_mix=1.0, recons=True)[0]
    assert dev_equal(r1["decoded"], r1["recons"]) and dev_equal(r1["converted"], r["converted"])


def test_engine_refuses_a_bank_of_another_model(engine):
    e = engine
    b = e["bank"]
    other_T = e["convert"].StyleBank(b.names, b.sums, b.counts, 2 * T, b.hop, b.S, b.checkpoint)
    with pytest.raises(ValueError, match="T=128"):
        e["conv"].convert(e["sources"], "a", other_T)
    other_S = e["convert"].StyleBank(b.names, b.sums[:, :4], b.counts, T, b.hop, 2, b.checkpoint)
    with pytest.raises(ValueError):
        e["conv"].convert(e["sources"], "a", other_S)
    with pytest.raises(KeyError):
        e["conv"].convert(e["sources"], "nobody", b)
    with pytest.raises(ValueError):
        e["conv"].convert(e["sources"], "a", b, style_mix=1.5)
    with pytest.raises(ValueError):
        e["convert"].Converter(e["tr"], hop=T + 1)


# -------------------------------------------------------------------------------------------------------------- command
def _cli(argv, timeout=600):
    """`python -m dvae_amd.convert` in a fresh child process under a time limit (kernel_harness.child starts the train and
    probe modules only; this is the same call for the new module)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = "import dvae_amd.convert as t, sys; sys.exit(t.main(sys.argv[1:]))"
    return subprocess.run([sys.executable, "-c", code] + [str(a) for a in argv], env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_train_convert_overlap_runs_the_engine_on_corpus_files(tmp_path):
    from kernel_harness import child
    from dvae_amd import convert
    rs = np.random.RandomState(3)
    corpus = tmp_path / "corpus"
    lengths = {"spkA": (150, 64), "spkB": (90, 70, 130)}
    for spk, ns in lengths.items():
        (corpus / spk).mkdir(parents=True)
        for u, n in enumerate(ns):
            np.save(corpus / spk / f"{spk}_u{u}_mel.npy", rs.rand(80, n).astype(F32))
    log = tmp_path / "results"
    (log / "checkpoints").mkdir(parents=True)
    torch.manual_seed(0)
    vsc = dvae_amd.ConvolutionalMulVAE("VCTK", 64, 80, 32, 1e-4, 0.01, 500, False, batch_size=2, speaker_size=4,
                                       device=torch.device("cuda"), latent_dim=32)
    torch.save(vsc.model.state_dict(), log / "checkpoints" / "DisentangledVAE_VCTK_0.pth")
    child("train", ["--convert", "True", f"--dataset_fp={corpus}", f"--log_dir={log}", "--src_spk=spkA", "--trg_spk=spkB",
                    "--batch-size=2", "--latent-size=32", "--speaker_size=4", "--griffin-lim-iters=2", "--overlap=16",
                    "--trg-utts=2", "--style-mix=0.8"])
    out = log / "generation" / "spkA_to_spkB"
    load = lambda spk: [np.load(p) for p in sorted((corpus / spk).glob("*.npy"))]
    conv = convert.Converter(vsc, hop=16, batch=32)
    want = conv.convert(load("spkA"), "spkB", conv.style_bank({"spkB": load("spkB")[:2]}), style_mix=0.8, recons=True)
    for u, (n, w_) in enumerate(zip(lengths["spkA"], want)):
        got = np.load(out / f"convert_spkA_to_spkB_u{u}.npy")
        assert got.shape == (80, n) and np.array_equal(got, w_["converted"].cpu().numpy()), "the same engine, the same bits"
        assert np.array_equal(np.load(out / f"recons_spkA_u{u}.npy"), w_["recons"].cpu().numpy())
        assert np.load(out / f"source_spkA_u{u}.npy").shape == (80, n)
        with wave.open(str(out / f"convert_spkA_to_spkB_u{u}.wav"), "rb") as w:
            assert (w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()) == (16000, 1, 2, (n - 3) * 256)
    cfg = json.load(open(log / "config.json"))
    assert cfg["overlap"] == 16 and cfg["trg_utts"] == 2 and cfg["style_mix"] == 0.8


def _frames(n, hop=256):
    return n // hop + (3 if n % hop == 0 else 4)


def test_command_wav_to_wav(tmp_path):
    from dvae_amd.preprocess import resample_lengths
    from dvae_amd.train import write_wav
    run = tmp_path / "run"
    (run / "checkpoints").mkdir(parents=True)
    (run / "config.json").write_text(json.dumps(dict(samples_length=64, latent_size=32, speaker_size=4, lr=1e-4, batch_size=4,
                                                     mse_cof=10, kl_cof=10)))
    torch.manual_seed(0)
    vsc = dvae_amd.ConvolutionalMulVAE("VCTK", 64, 80, 32, 1e-4, 0.01, 500, False, batch_size=4, speaker_size=4,
                                       device=torch.device("cuda"), latent_dim=32)
    torch.save(vsc.model.state_dict(), run / "checkpoints" / "DisentangledVAE_VCTK_2.pth")
    del vsc
    src, trg, out = tmp_path / "src", tmp_path / "trg", tmp_path / "out"
    src.mkdir(), trg.mkdir()
    t22 = np.arange(int(0.9 * 22050)) / 22050.0
    write_wav(str(src / "sweep.wav"), 0.4 * np.sin(2 * np.pi * (200.0 + 900.0 * t22) * t22), 22050)
    t16 = np.arange(int(0.5 * 16000)) / 16000.0
    write_wav(str(src / "tone.wav"), 0.3 * np.sin(2 * np.pi * 330.0 * t16), 16000)
    write_wav(str(src / "silent.wav"), np.zeros(8000), 16000)
    tt = np.arange(16000) / 16000.0
    write_wav(str(trg / "t1.wav"), 0.3 * np.sin(2 * np.pi * 150.0 * tt) + 0.1 * np.sin(2 * np.pi * 450.0 * tt), 16000)
    write_wav(str(trg / "t2.wav"), 0.3 * np.sin(2 * np.pi * 180.0 * tt[:12000]), 16000)
    base = ["--log_dir", run, "--griffin-lim-iters", 2, "--batch", 4, "-o", out]
    r = _cli(base + ["--source", src, "--target", trg / "t1.wav", trg / "t2.wav"])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "silent.wav" in r.stderr and "silent" in r.stderr.split("silent.wav", 1)[1].splitlines()[0], r.stderr[-1500:]
    assert sorted(p.name for p in out.iterdir()) == ["convert_sweep.npy", "convert_sweep.wav", "convert_tone.npy",
                                                     "convert_tone.wav"]
    n_sweep = int(resample_lengths(len(t22), 22050)[1])
    assert n_sweep == 14400
    for stem, n in (("sweep", n_sweep), ("tone", 8000)):
        with wave.open(str(out / f"convert_{stem}.wav"), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, n)
        mel = np.load(out / f"convert_{stem}.npy")
        assert mel.shape == (80, _frames(n)) and mel.dtype == F32 and np.isfinite(mel).all()
        assert mel.min() >= 0.0 and mel.max() <= 1.0
    # only silent targets: nothing to take a style from
    write_wav(str(trg / "quiet.wav"), np.zeros(6000), 16000)
    r = _cli(base + ["--source", src / "tone.wav", "--target", trg / "quiet.wav"])
    assert r.returncode != 0 and "no usable --target" in r.stderr, (r.returncode, r.stderr[-1500:])
