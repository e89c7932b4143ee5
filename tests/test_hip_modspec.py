"""Over-smoothing instruments on the MI355X: the kernels of csrc/modspec.hip (dvae_mel_gv, dvae_modspec_windows,
dvae_modspec_group_sum, dvae_modspec_filter) through the C ABI against the float64 restatement of tests/modspec_ref.py, then
dvae_amd.modspec.ModSpec, the switch in dvae_amd.convert.Converter and the two commands.

Every launch writes into guarded buffers of tests/kernel_harness.py filled with 0xFF; inputs carry NaN wherever a launch must
not read (around the windows, in the columns of the packed mels that no utterance owns).  The inputs are seeded random
trajectories for which the restatement keeps |Y_k| >= 1e-6 sum|d_t| at EVERY element — asserted here on the CPU side — so every
element is compared with its derived bound; what the restatement derives as bits (group sums of the device's own rows, alpha
= 0, short utterances, columns nobody owns, a second launch) is compared bit for bit.
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
from kernel_harness import (assert_same_bits, Buf, dev_equal, EINVAL, F32, F64, guards, ibuf, L, ok, Pad, ROOT, st,  # noqa: E402
                            untouched, Worst)
import dvae_amd  # noqa: E402,F401
import convert_ref as CR  # noqa: E402
import modspec_ref as M  # noqa: E402

WORST = Worst("test_hip_modspec.py", sort=True)
note = WORST.note
I32 = np.int32
DS, CS, NS = (8, 64, 128), (1, 3, 80), (1, 2, 65)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def _rng(*key):
    return np.random.RandomState(1000003 + sum(31 ** i * int(k) for i, k in enumerate(key)))


def _held(windows):
    """the condition under which no element is exempt: a seed that violates it is a wrong seed"""
    _, d, Y = M.analyse(windows)
    r = M.ratio(d, Y)
    assert (r >= M.MIN_RATIO).all(), f"|Y_k| / sum|d_t| = {r.min():.3g} < {M.MIN_RATIO}: choose another seed"


def _stats(rng, C, D):
    """natural and generated statistics [C, D/2] of a few windows each (the generated ones smoothed)"""
    nat = M.trajectories(rng, (4, C, D))
    gen = M.attenuate(M.trajectories(rng, (4, C, D)), np.linspace(0.9, 0.3, D // 2)).astype(F32)
    return M.window_stats(nat) + M.window_stats(gen)


def _filter(win_ptr, nwin, C, D, tw, stats, alpha, gain, out):
    return L().dvae_modspec_filter(win_ptr, nwin, C, D, tw.ptr, *(s.ptr for s in stats), alpha, gain, out.ptr, st())


# -------------------------------------------------------------------------------------- windows and filter, dense shapes
@pytest.mark.parametrize("nwin", NS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("D", DS)
def test_windows_and_filter(D, C, nwin):
    rng = _rng(D, C, nwin)
    w = M.trajectories(rng, (nwin, C, D))
    _held(w)
    win, tw = Pad(w), Buf(data=M.twiddle(D))
    rows = Buf((nwin * C, D))
    ok(L().dvae_modspec_windows(win.ptr, nwin, C, D, tw.ptr, rows.ptr, st()), "dvae_modspec_windows")
    guards(rows, win.buf, tw)
    ref, tol = M.rows(w)
    got = rows.np()
    note(("modspec_windows s", f"D{D}"), got[:, :D // 2], ref[:, :D // 2], tol[:, :D // 2], "s")
    note(("modspec_windows s^2", f"D{D}"), got[:, D // 2:], ref[:, D // 2:], tol[:, D // 2:], "s^2")
    assert_same_bits(got[:, D // 2:], (got[:, :D // 2].astype(F64) ** 2).astype(F32), "s^2 is the stored s squared, rounded once")
    again = Buf((nwin * C, D))
    ok(L().dvae_modspec_windows(win.ptr, nwin, C, D, tw.ptr, again.ptr, st()))
    assert np.array_equal(rows.bits(), again.bits()), "a second launch gives the same bits"

    stats = _stats(rng, C, D)
    sb = [Buf(data=s) for s in stats]
    for alpha, gain in ((1.0, 12.0), (0.4, 3.0)):
        out = Buf((nwin, C, D))
        ok(_filter(win.ptr, nwin, C, D, tw, sb, alpha, gain, out), "dvae_modspec_filter")
        guards(out, win.buf, tw, *sb)
        yref, ytol = M.filter_windows(w, *stats, alpha, gain)
        note((f"modspec_filter alpha {alpha}", f"D{D}"), out.np(), yref, ytol, "filter")
        out2 = Buf((nwin, C, D))
        ok(_filter(win.ptr, nwin, C, D, tw, sb, alpha, gain, out2))
        assert np.array_equal(out.bits(), out2.bits()), "a second launch gives the same bits"
    out = Buf((nwin, C, D))
    ok(_filter(win.ptr, nwin, C, D, tw, sb, 0.0, 12.0, out))
    guards(out)
    assert_same_bits(out, w, "alpha = 0 is a copy")


# ------------------------------------------------------------------------------------------------------ the packed batch
def _batch(D, C):
    """utterances of D - 1, D, D + 1, 2 D - 1 and 3 D + 5 frames in one packed buffer, NaN in the columns nobody owns; the
    window of the short one is a padding window of the list"""
    rng = _rng(D, C, 7)
    lengths = M.case_lengths(D)
    utt, win, ld, nreal = M.cut(lengths, D, D // 2)
    assert nreal == len(win) - 1 and win[0][0] == -1 and utt[0][3] == 0
    mels = np.full((C, ld), np.nan, F32)
    for col0, n, _, _ in utt:
        mels[:, col0:col0 + n] = M.trajectories(rng, (C, n))
    return dict(rng=rng, utt=utt, win=win, ld=ld, mels=mels, lengths=lengths)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("D", DS)
def test_mel_gv(D, C):
    b = _batch(D, C)
    mels, utt = Buf(data=b["mels"]), ibuf(b["utt"], I32)
    out = Buf((len(b["utt"]), C, 2), torch.float64)
    args = (mels.ptr, b["ld"], utt.ptr, len(b["utt"]), C)
    ok(L().dvae_mel_gv(*args, out.ptr, st()), "dvae_mel_gv")
    guards(out, mels, utt)
    ref = M.gv(b["mels"], b["utt"])
    got = out.np()
    note(("mel_gv mean", f"D{D}"), got[..., 0], ref["m"], ref["tol_m"], "mean")
    note(("mel_gv variance", f"D{D}"), got[..., 1], ref["v"], ref["tol_v"], "variance")
    assert (got[..., 1] > 0).all()
    out2 = Buf((len(b["utt"]), C, 2), torch.float64)
    ok(L().dvae_mel_gv(*args, out2.ptr, st()))
    assert np.array_equal(out.bits(), out2.bits()), "a second launch gives the same bits"


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("D", DS)
def test_packed_batch_rows_sums_filter_and_overlap_add(D, C):
    b = _batch(D, C)
    utt_h, win_h, ld = b["utt"], b["win"], b["ld"]
    n = len(win_h)
    mels, utt, win, tw = Buf(data=b["mels"]), ibuf(utt_h, I32), ibuf(win_h, I32), Buf(data=M.twiddle(D))
    wins = Buf((n, C, D))
    ok(L().dvae_mel_to_windows(mels.ptr, ld, utt.ptr, win.ptr, wins.ptr, n, C, D, st()))
    w = wins.np()
    assert_same_bits(w, M.windows_of(np.nan_to_num(b["mels"]), utt_h, win_h, D), "the cut")
    assert not w[0].any(), "the short utterance's window is a padding window: zeros"
    _held(w[1:])
    rows = Buf((n * C, D))
    ok(L().dvae_modspec_windows(wins.ptr, n, C, D, tw.ptr, rows.ptr, st()))
    guards(rows, wins)
    got = rows.np().reshape(n, C, D)
    ref, tol = (a.reshape(n, C, D) for a in M.rows(w))
    note(("modspec_windows s", f"D{D}"), got[1:], ref[1:], tol[1:], "rows of the packed batch")
    floor = np.asarray(np.log(M.FLOOR), F64).astype(F32)
    assert_same_bits(got[0, :, :D // 2], np.full((C, D // 2), floor), "a padding window's rows: ln FLOOR")

    # group sums: two groups over the real windows in turn, the padding window in none; an index out of range is passed over
    real = np.arange(1, n)
    order = np.concatenate([real[0::2], [-1, n], real[1::2]]).astype(I32)
    first = np.asarray([0, len(real[0::2]) + 2, len(order)], I32)
    ob, fb = ibuf(order, I32), ibuf(first, I32)
    sums = Buf((2, C, D), torch.float64)
    args = (rows.ptr, ob.ptr, len(order), fb.ptr, 2, n, C, D)
    ok(L().dvae_modspec_group_sum(*args, sums.ptr, st()), "dvae_modspec_group_sum")
    guards(sums, rows, ob, fb)
    want = M.group_sum(rows.np(), order, first, C)
    assert np.array_equal(sums.np().view(np.int64), want.view(np.int64)), "the sequential float64 sum of the device's own rows"
    sums2 = Buf((2, C, D), torch.float64)
    ok(L().dvae_modspec_group_sum(*args, sums2.ptr, st()))
    assert np.array_equal(sums.bits(), sums2.bits())

    # filter and cross-fade back: the bound where a window was filtered, the fill everywhere else
    stats = _stats(b["rng"], C, D)
    sb = [Buf(data=s) for s in stats]
    y = Buf((n, C, D))
    ok(_filter(wins.ptr, n, C, D, tw, sb, 1.0, 12.0, y))
    guards(y)
    yref, ytol = M.filter_windows(w, *stats, 1.0, 12.0)
    note(("modspec_filter alpha 1.0", f"D{D}"), y.np(), yref, ytol, "filter of the packed batch")
    assert not y.bits()[0].any(), "a padding window stays +0.0"
    w32 = Buf(data=CR.window(D).astype(F32))
    out = Buf((C, ld))
    ok(L().dvae_windows_overlap_add(y.ptr, utt.ptr, win.ptr, w32.ptr, out.ptr, ld, len(utt_h), C, D, 0.0, 1.0, 1, st()))
    guards(out)
    oref, otol, written = M.overlap_add(yref, ytol, utt_h, win_h, CR.window(D).astype(F32), np.zeros((C, ld), F32))
    col0, n0 = utt_h[0][0], utt_h[0][1]
    assert not written[:, col0:col0 + n0].any() and written.sum() == C * sum(b["lengths"][1:])
    untouched(out.bits()[~written], "columns no utterance owns, and the utterance shorter than D")
    note(("filter + overlap_add", f"D{D}"), out.np()[written], oref[written], otol[written], "cross-faded back")


# ----------------------------------------------------------------------------------------------------------------- EINVAL
def test_einval_launches_nothing():
    D, C, n = 8, 3, 2
    rng = _rng(1)
    w = Pad(M.trajectories(rng, (n, C, D)))
    tw = Buf(data=np.concatenate([M.twiddle(D).reshape(-1), [0.0]]))
    stats = [Buf(data=np.concatenate([s.reshape(-1), [0.0]])) for s in _stats(rng, C, D)]
    rows, y = Buf((n * C, D)), Buf((n, C, D))
    good = [w.ptr, n, C, D, tw.ptr, rows.ptr]
    for i, bad in ((0, None), (4, None), (5, None), (1, 0), (1, -1), (2, 0), (3, 0), (3, 6), (3, 9), (3, 130), (3, 7),
                   (4, tw.ptr + 4)):
        a = list(good)
        a[i] = bad
        assert L().dvae_modspec_windows(*a, st()) == EINVAL, ("windows", i, bad)
    untouched(rows.bits(), "modspec_windows after EINVAL")
    good = [w.ptr, n, C, D, tw.ptr] + [s.ptr for s in stats] + [1.0, 12.0, y.ptr]
    cases = [(i, None) for i in (0, 4, 5, 6, 7, 8, 11)] + [(1, 0), (2, 0), (2, -3), (3, 0), (3, 9), (3, 130), (3, 4)]
    cases += [(9, -0.1), (9, 1.5), (9, float("nan")), (10, 0.0), (10, -12.0), (10, float("nan")), (11, w.ptr)]
    cases += [(i, good[i] + 4) for i in (4, 5, 6, 7, 8)]
    for i, bad in cases:
        a = list(good)
        a[i] = bad
        assert L().dvae_modspec_filter(*a, st()) == EINVAL, ("filter", i, bad)
    untouched(y.bits(), "modspec_filter after EINVAL")
    utt = ibuf(np.asarray([[0, 12, 0, 2]]), I32)
    mels = Buf(data=M.trajectories(rng, (C, 12)))
    gv = Buf((2, C, 2), torch.float64)
    good = [mels.ptr, 12, utt.ptr, 1, C, gv.ptr]
    for i, bad in ((0, None), (2, None), (5, None), (1, 0), (3, 0), (4, 0), (4, -1), (5, gv.ptr + 4)):
        a = list(good)
        a[i] = bad
        assert L().dvae_mel_gv(*a, st()) == EINVAL, ("gv", i, bad)
    untouched(gv.bits().view(np.int32), "mel_gv after EINVAL")
    order, first = ibuf([0, 1], I32), ibuf([0, 2], I32)
    rr = Buf(data=np.zeros((n * C, D), F32))
    sums = Buf((2, C, D), torch.float64)
    good = [rr.ptr, order.ptr, 2, first.ptr, 1, n, C, D, sums.ptr]
    for i, bad in ((0, None), (1, None), (3, None), (8, None), (2, 0), (4, 0), (5, 0), (6, 0), (7, 7), (7, 130), (8, sums.ptr + 4)):
        a = list(good)
        a[i] = bad
        assert L().dvae_modspec_group_sum(*a, st()) == EINVAL, ("group_sum", i, bad)
    untouched(sums.bits().view(np.int32), "modspec_group_sum after EINVAL")
    # a table entry that does not fit the packed buffer: NaN, nothing read
    bad_utt = ibuf(np.asarray([[0, 12, 0, 0], [8, 12, 0, 0], [-4, 4, 0, 0], [0, 0, 0, 0]]), I32)
    out = Buf((4, C, 2), torch.float64)
    ok(L().dvae_mel_gv(mels.ptr, 12, bad_utt.ptr, 4, C, out.ptr, st()))
    guards(out, mels)
    got = out.np()
    assert np.isfinite(got[0]).all() and np.isnan(got[1:]).all()


# ------------------------------------------------------------------------------------------------------------- the engine
def _ms(D, hop=None):
    from dvae_amd import modspec
    return modspec, modspec.ModSpec(torch.device("cuda"), D, hop)


def test_stats_follow_the_restatement():
    modspec, ms = _ms(16)
    rng = _rng(2)
    groups = {"a": [M.trajectories(rng, (5, n)) for n in (40, 9, 16)], "b": [M.trajectories(rng, (5, 33))],
              "short": [M.trajectories(rng, (5, 15))]}
    got = ms.stats(groups)
    ref = M.group_stats(groups, 16, 8)
    assert got.names == ref["names"] and (got.D, got.hop, got.C) == (16, 8, 5)
    assert got.windows.tolist() == ref["windows"].tolist() == [5, 4, 0] and got.utterances.tolist() == [2, 1, 0]
    for k in ("s_sum", "s_sq", "v_sum", "lnv_sum"):
        note((f"stats {k}", "D16"), getattr(got, k)[:2], ref[k][:2], ref["tol_" + k][:2], k)
        assert not getattr(got, k)[2].any()
    with pytest.raises(ValueError, match="no window"):
        got.mean("short")
    again = ms.stats(groups)
    assert all(np.array_equal(getattr(got, k), getattr(again, k)) for k in ("s_sum", "s_sq", "v_sum", "lnv_sum"))
    sc = ms.score(got, "a", got, "b")
    want = M.score(got.mean("a"), got.log_gv("a"), got.mean("b"), got.log_gv("b"))
    assert sc["msd_db"] == pytest.approx(want["msd_db"], rel=1e-13) and sc["gv_ratio_db"] == pytest.approx(want["gv_ratio_db"], rel=1e-12)
    assert np.allclose(sc["frequencies_hz"], M.frequencies(16)) and sc["profile"].shape == (8,)


def test_postfilter_bounds_and_bits():
    modspec, ms = _ms(8)
    rng = _rng(3)
    mels = [M.trajectories(rng, (4, n)) for n in M.case_lengths(8)]
    nat = ms.stats({"n": [M.trajectories(rng, (4, 90))]})
    gen = ms.stats({"g": [M.attenuate(M.trajectories(rng, (4, 90)), 0.5).astype(F32)]})
    zero = ms.postfilter(mels, (nat, "n"), (gen, "g"), alpha=0.0)
    assert all(dev_equal(z, torch.from_numpy(m).cuda()) for z, m in zip(zero, mels)), "alpha = 0: the input's bits"
    for alpha, gain in ((1.0, 12.0), (0.5, 2.0)):
        got = ms.postfilter(mels, (nat, "n"), (gen, "g"), alpha=alpha, max_gain_db=gain)
        ref = M.postfilter(mels, 8, 4, nat.mean("n"), nat.std("n"), gen.mean("g"), gen.std("g"), alpha, gain)
        assert dev_equal(got[0], torch.from_numpy(mels[0]).cuda()), "an utterance shorter than D keeps its bits"
        for g, (r, t), m in zip(got[1:], ref[1:], mels[1:]):
            assert tuple(g.shape) == m.shape and float(g.min()) >= 0.0 and float(g.max()) <= 1.0
            note((f"postfilter alpha {alpha}", "D8"), g.cpu().numpy(), r, t, "ModSpec.postfilter")
    with pytest.raises(ValueError):
        ms.postfilter(mels, (nat, "n"), (gen, "g"), alpha=1.5)
    with pytest.raises(ValueError):
        ms.postfilter(mels, (nat, "n"), (gen, "g"), max_gain_db=0.0)
    with pytest.raises(ValueError, match="D=16"):
        ms.postfilter(mels, (_ms(16)[1].stats({"n": [M.trajectories(rng, (4, 40))]}), "n"), (gen, "g"))


def test_restoration_on_the_device():
    D, C = 16, 5
    modspec, ms = _ms(D, hop=D)
    rng = _rng(4)
    nat = M.trajectories(rng, (14, C, D))
    a = rng.uniform(0.3, 1.0, D // 2)
    gen = M.attenuate(nat, a).astype(F32)
    _held(nat), _held(gen)
    join = lambda w: [np.ascontiguousarray(np.concatenate(list(w[:8]), 1)), np.ascontiguousarray(np.concatenate(list(w[8:]), 1))]
    utt_n, utt_g = join(nat), join(gen)
    sn, sg = ms.stats({"natural": utt_n}), ms.stats({"generated": utt_g})
    assert sn.windows.tolist() == sg.windows.tolist() == [14]
    back = ms.postfilter(utt_g, (sn, "natural"), (sg, "generated"), alpha=1.0)
    tol = join(M.restoration_tol(nat, gen, a))
    for b, want, t in zip(back, utt_n, tol):
        assert t.max() < 2.0 ** -8, "the derived bound stays far below a bf16-level error"
        note(("restoration", "D16"), b.cpu().numpy(), want, t, "the natural mel comes back")
    before = ms.score(sg, "generated", sn, "natural")
    after = ms.score(ms.stats({"filtered": back}), "filtered", sn, "natural")
    assert after["msd_db"] < 1e-3 * before["msd_db"] and before["msd_db"] > 1.0
    assert before["gv_ratio_db"] < -0.5 and abs(after["gv_ratio_db"]) < 1e-3


T, BATCH, LENGTHS = 64, 4, (150, 64, 40)


@pytest.fixture(scope="module")
def engine():
    from dvae_amd import convert, modspec
    torch.manual_seed(0)
    tr = dvae_amd.ConvolutionalMulVAE("VCTK", T, 80, 32, 1e-4, 0.01, 500, False, batch_size=BATCH, speaker_size=4,
                                      device=torch.device("cuda"), latent_dim=32, mse_cof=10, kl_cof=10)
    rs = np.random.RandomState(7)
    sources = [M.trajectories(rs, (80, n)) for n in LENGTHS]
    targets = {"a": [M.trajectories(rs, (80, 100)), M.trajectories(rs, (80, 70))], "b": [M.trajectories(rs, (80, 64))]}
    conv = convert.Converter(tr, batch=BATCH)
    bank = conv.style_bank(targets)
    ms = modspec.ModSpec(torch.device("cuda"), 32)
    return dict(tr=tr, conv=conv, sources=sources, targets=targets, bank=bank, ms=ms)


def test_engine_without_postfilter_keeps_its_bits(engine):
    from test_hip_convert import _by_hand
    e = engine
    names = ["a", "b", "a"]
    plain = e["conv"].convert(e["sources"], names, e["bank"], style_mix=0.6)
    none = e["conv"].convert(e["sources"], names, e["bank"], style_mix=0.6, postfilter=None)
    hand, _ = _by_hand(e["tr"], e["sources"], e["bank"].sums, e["bank"].counts, [0, 1, 0], 0.6, T // 2, BATCH)
    for p, q, h in zip(plain, none, hand):
        assert sorted(p) == ["converted"] and dev_equal(p["converted"], q["converted"])
        assert dev_equal(p["converted"], h), "the launches of the conversion chain as they were, composed by hand"


def test_engine_with_postfilter_is_the_hand_composed_launches(engine):
    e = engine
    ms, conv, names = e["ms"], e["conv"], ["a", "b", "a"]
    natural, generated = conv.smoothing_stats(e["targets"], e["bank"], ms)
    assert natural.names == generated.names == ["a", "b"] and natural.D == 32
    assert natural.windows.tolist() == generated.windows.tolist() == [6 + 4, 3] and generated.utterances.tolist() == [2, 1]
    own = {n: [r["converted"] for r in conv.convert(e["targets"][n], n, e["bank"])] for n in e["targets"]}
    again = ms.stats(own)
    assert all(np.array_equal(getattr(generated, k), getattr(again, k)) for k in ("s_sum", "s_sq", "v_sum", "lnv_sum"))
    plain = conv.convert(e["sources"], names, e["bank"], style_mix=0.6)
    got = conv.convert(e["sources"], names, e["bank"], style_mix=0.6, postfilter=(ms, natural, generated, 0.8, 6.0))
    for g, n in zip(got, LENGTHS):
        y = g["converted"]
        assert tuple(y.shape) == (80, n) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
        assert float(y.min()) >= 0.0 and float(y.max()) <= 1.0
    # by hand: per target name the plain conversions packed, cut, dvae_modspec_filter, dvae_windows_overlap_add
    lib, dev = L(), "cuda"
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    for name in ("a", "b"):
        idx = [i for i, n in enumerate(names) if n == name]
        mels = [plain[i]["converted"] for i in idx]
        utt, win, ld, _ = M.cut([int(m.shape[1]) for m in mels], 32, 16)
        packed = torch.zeros((80, ld), device=dev)
        for m, (col0, n_fr, _, _) in zip(mels, utt):
            packed[:, col0:col0 + n_fr] = m
        utt_d, win_d, n = up(utt, I32), up(win, I32), len(win)
        x, y = torch.empty((n, 80, 32), device=dev), torch.empty((n, 80, 32), device=dev)
        ok(lib.dvae_mel_to_windows(packed.data_ptr(), ld, utt_d.data_ptr(), win_d.data_ptr(), x.data_ptr(), n, 80, 32, st()))
        stats = [up(s, F64) for s in (natural.mean(name), natural.std(name), generated.mean(name), generated.std(name))]
        tw = up(M.twiddle(32), F64)
        ok(lib.dvae_modspec_filter(x.data_ptr(), n, 80, 32, tw.data_ptr(), *(s.data_ptr() for s in stats), 0.8, 6.0,
                                   y.data_ptr(), st()))
        out, w32 = packed.clone(), up(CR.window(32), F32)
        ok(lib.dvae_windows_overlap_add(y.data_ptr(), utt_d.data_ptr(), win_d.data_ptr(), w32.data_ptr(), out.data_ptr(), ld,
                                        len(utt), 80, 32, 0.0, 1.0, 1, st()))
        for i, (col0, n_fr, _, _) in zip(idx, utt):
            assert dev_equal(got[i]["converted"], out[:, col0:col0 + n_fr].contiguous()), (name, i)
    assert not dev_equal(got[0]["converted"], plain[0]["converted"]) or float(plain[0]["converted"].std()) == 0.0


# --------------------------------------------------------------------------------------------------------------- commands
def _cli(module, argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = f"import dvae_amd.{module} as t, sys; sys.exit(t.main(sys.argv[1:]))"
    return subprocess.run([sys.executable, "-c", code] + [str(a) for a in argv], env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_commands(tmp_path):
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
    src, trg = tmp_path / "src", tmp_path / "trg"
    src.mkdir(), trg.mkdir()
    t = np.arange(16000) / 16000.0
    write_wav(str(src / "sweep.wav"), 0.4 * np.sin(2 * np.pi * (200.0 + 900.0 * t) * t), 16000)
    write_wav(str(src / "tone.wav"), 0.3 * np.sin(2 * np.pi * 330.0 * t[:9000]) * (1 + 0.5 * np.sin(2 * np.pi * 7.0 * t[:9000])), 16000)
    write_wav(str(trg / "t1.wav"), 0.3 * np.sin(2 * np.pi * 150.0 * t) * (1 + 0.6 * np.sin(2 * np.pi * 5.0 * t)), 16000)
    write_wav(str(trg / "t2.wav"), 0.3 * np.sin(2 * np.pi * (180.0 + 60.0 * t[:12000]) * t[:12000]), 16000)
    write_wav(str(trg / "brief.wav"), 0.3 * np.sin(2 * np.pi * 220.0 * t[:1500]), 16000)
    outs = [tmp_path / f"out{i}" for i in range(3)]
    base = ["--log_dir", run, "--griffin-lim-iters", 2, "--batch", 4, "--source", src, "--target", trg]
    for out, extra in zip(outs, ([], [], ["--ms-postfilter", 0.7, "--ms-window", 16, "--ms-max-gain-db", 9])):
        r = _cli("convert", base + ["-o", out] + extra)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    names = ["convert_sweep.npy", "convert_sweep.wav", "convert_tone.npy", "convert_tone.wav"]
    for out in outs:
        assert sorted(p.name for p in out.iterdir()) == names
    for name in names:
        assert (outs[0] / name).read_bytes() == (outs[1] / name).read_bytes(), f"{name}: two runs without the flag differ"
    for stem, n in (("sweep", 16000), ("tone", 9000)):
        with wave.open(str(outs[2] / f"convert_{stem}.wav"), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, n)
        a, b = np.load(outs[0] / f"convert_{stem}.npy"), np.load(outs[2] / f"convert_{stem}.npy")
        assert a.shape == b.shape and b.dtype == F32 and np.isfinite(b).all() and b.min() >= 0.0 and b.max() <= 1.0
    # the score command on what was written, against the targets
    r = _cli("modspec", ["score", outs[2], trg, "--D", 16])
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    lines = lines[next(i for i, ln in enumerate(lines) if ln.startswith("msd: ")):]
    assert lines[0].startswith("msd: ") and lines[0].endswith(" dB") and lines[1].startswith("gv ratio: ")
    assert sum(ln.startswith("profile ") for ln in lines) == 8
    res = json.loads((outs[2] / "modspec.json").read_text())
    assert res["D"] == 16 and res["utterances"] == {"converted": 2, "natural": 2} and len(res["profile"]) == 8
    assert np.isfinite([res["msd_db"], res["gv_ratio_db"]]).all() and float(lines[0].split()[1]) == res["msd_db"]
    assert [os.path.basename(p) for p in res["too_short"]["natural"]] == ["brief.wav"] and res["too_short"]["converted"] == []
    assert "brief.wav" in r.stderr
