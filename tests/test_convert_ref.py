"""CPU checks of whole-utterance conversion's host side: the window plan of dvae_amd/convert.py against its properties and
against the restatement of tests/convert_ref.py, the cross-fade window, the identity cut -> overlap-add, and the mutations
the restatement's comparison (`close`, `latents_close`: bits where it says bits, the derived bound elsewhere) must catch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import convert_ref as R  # noqa: E402

F32, F64 = np.float32, np.float64


def _convert():
    import dvae_amd  # noqa: F401
    from dvae_amd import convert
    return convert


# ------------------------------------------------------------------------------------------------------------------ plan
@pytest.mark.parametrize("L,T,hop", R.GRID, ids=lambda v: str(v))
def test_plan_properties(L, T, hop):
    starts = _convert().window_plan(L, T, hop)
    assert starts.dtype == np.int64 and starts.tolist() == R.window_starts(L, T, hop)
    assert (R.cover_counts(L, T, starts) >= 1).all(), "a frame below L is not covered"
    assert starts.min() >= 0 and starts.max() <= max(0, L - T)
    assert (np.diff(starts) > 0).all()
    if L >= T:
        assert starts[-1] + T == L
    else:
        assert starts.tolist() == [0]
    if hop == T and L % T == 0:
        assert starts.tolist() == list(range(0, L, T)) and (R.cover_counts(L, T, starts) == 1).all()


def test_plan_refuses_bad_arguments():
    c = _convert()
    for bad in ((0, 4, 2), (5, 4, 0), (5, 4, 5), (5, 0, 1)):
        with pytest.raises(ValueError):
            c.window_plan(*bad)
    with pytest.raises(ValueError):
        c.flat_plan([], 4, 2)


@pytest.mark.parametrize("T", [4, 8, 64])
def test_crossfade_window(T):
    w = _convert().crossfade_window(T)
    assert w.dtype == F64 and w.shape == (T,)
    np.testing.assert_allclose(w, R.window(T), rtol=0, atol=2 ** -50)
    assert (w > 0).all() and (w.astype(F32) > 0).all()
    np.testing.assert_allclose(w, w[::-1], rtol=0, atol=2 ** -50)
    np.testing.assert_allclose(w[:T // 2] + w[T // 2:], 1.0, rtol=0, atol=2 ** -50)      # partition of unity at hop = T / 2
    L = 5 * T                                    # ... and so the overlap-added window is 1 away from the two ends
    den = np.zeros(L)
    for s in R.window_starts(L, T, T // 2):
        den[s:s + T] += w
    np.testing.assert_allclose(den[T // 2:L - T // 2], 1.0, rtol=0, atol=2 ** -48)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_flat_plan_matches_the_restatement(c):
    p = _convert().flat_plan(c["lengths"], c["T"], c["hop"], c["batch"])
    utt, win, ld, nwin = R.plan(c["lengths"], c["T"], c["hop"], c["batch"])
    assert p["utt"].dtype == np.int32 and p["win"].dtype == np.int32
    assert np.array_equal(p["utt"], utt) and np.array_equal(p["win"], win) and p["ld"] == ld and p["nwin"] == nwin
    assert (p["utt"][:, 0] % 4 == 0).all() and len(p["win"]) % c["batch"] == 0 and len(p["win"]) > nwin
    assert (p["win"][nwin:, 0] == -1).all() and (p["win"][:nwin, 0] >= 0).all()
    # the windows of an utterance are contiguous and sorted; utterances do not overlap
    for u, (col0, L, win0, nw) in enumerate(p["utt"]):
        assert (p["win"][win0:win0 + nw, 0] == u).all() and (np.diff(p["win"][win0:win0 + nw, 1]) > 0).all()
        assert u == 0 or col0 >= p["utt"][u - 1][0] + p["utt"][u - 1][1]
    assert R.rows_of(len(win), c["batch"])[nwin - 1] == ((nwin - 1) // c["batch"], (nwin - 1) % c["batch"])


# ------------------------------------------------------------------------------------------------------------- identity
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_cut_and_overlap_add_is_the_identity(c):
    d = R.case_data(c)
    wins = R.mel_to_windows(d["mels"], d["utt"], d["win"], c["T"])
    assert np.isfinite(wins).all(), "a column no utterance owns was read into a window"
    assert not wins[d["nwin"]:].any(), "a padding window is all zeros"
    res = R.overlap_add(wins, d["utt"], d["win"], d["w32"], d["ld"])
    X = d["mels"]
    o, s = res["owned"], res["single"]
    assert np.array_equal(o, np.isfinite(X))
    assert np.array_equal(res["ref"][s].astype(F32).view(np.uint32), X[s].view(np.uint32)), "one window covers: bits"
    # every window holds X itself there, so num / den = X up to the restatement's own float64 roundings: inside the bound
    assert (np.abs(res["ref"][o] - X[o].astype(F64)) <= res["tol"][o]).all()
    assert R.close(X, res)


# ------------------------------------------------------------------------------------------------------------- mutations
def _ola(y, utt, win, w32, ld, normalise=True):
    """A plain overlap-add that takes a (mutated) plan as it comes: NaN where nothing covers."""
    y, w = np.asarray(y, F32), np.asarray(w32, F32).astype(F64)
    _, C, T = y.shape
    out = np.full((C, ld), np.nan, F64)
    for u, (col0, L, _, _) in enumerate(utt):
        for t in range(L):
            cover = [k for k in range(len(win)) if win[k][0] == u and win[k][1] <= t < win[k][1] + T]
            if not cover:
                continue
            if len(cover) == 1 and normalise:
                out[:, col0 + t] = y[cover[0], :, t - win[cover[0]][1]]
                continue
            num = sum(w[t - win[k][1]] * y[k, :, t - win[k][1]].astype(F64) for k in cover)
            den = sum(w[t - win[k][1]] for k in cover)
            out[:, col0 + t] = num / den if normalise else num
    return out.astype(F32)


MUT = dict(C=3, T=8, hop=7, lengths=(1, 9, 19), batch=4)       # hop = T - 1: the overlap-added window is far from 1


def _mut_setup():
    d = R.case_data(MUT)
    wins = R.mel_to_windows(d["mels"], d["utt"], d["win"], MUT["T"])
    res = R.overlap_add(wins, d["utt"], d["win"], d["w32"], d["ld"])
    return d, wins, res


def test_the_unmutated_path_passes():
    d, wins, res = _mut_setup()
    assert R.close(_ola(wins, d["utt"], d["win"], d["w32"], d["ld"]), res)


def test_mutation_moved_last_window_dropped():
    d, wins, res = _mut_setup()
    win = d["win"].copy()
    for col0, L, win0, nw in d["utt"]:
        if nw > 1:
            win[win0 + nw - 1, 0] = -1
    assert not R.close(_ola(wins, d["utt"], win, d["w32"], d["ld"]), res)


def test_mutation_frame0_off_by_one():
    d, _, res = _mut_setup()
    win = d["win"].copy()
    win[:d["nwin"], 1] += 1
    shifted = R.mel_to_windows(np.nan_to_num(d["mels"]), d["utt"], win, MUT["T"])
    assert not R.close(_ola(shifted, d["utt"], d["win"], d["w32"], d["ld"]), res)


def test_mutation_normalisation_left_out():
    d, wins, res = _mut_setup()
    assert not R.close(_ola(wins, d["utt"], d["win"], d["w32"], d["ld"], normalise=False), res)


def test_mutation_window_credited_to_the_neighbour():
    d, wins, res = _mut_setup()
    win = d["win"].copy()
    win0 = d["utt"][1][2]
    win[win0, 0] = 2                            # the first window of utterance 1 counted as one of utterance 2
    assert not R.close(_ola(wins, d["utt"], win, d["w32"], d["ld"]), res)


def test_latent_restatement_and_its_mutations():
    c = R.latent_case()
    S = c["S"]
    for mix in (0.0, 0.37, 1.0):
        z, tol = R.window_latents(c["content"], c["sums"], c["counts"], c["g_src"], c["g_trg"], mix, S)
        assert R.latents_close(z.astype(F32), z, tol)
        assert (tol[:, S:] == 0).all() and ((tol[:, :S] == 0).all() == (mix in (0.0, 1.0)))
        assert (tol <= np.spacing(np.abs(z).astype(F32)).astype(F64) + 2 ** -125).all(), "the bound stays under one fp32 ulp"
        assert not z[-1].any(), "a padding row is zero"
    assert 1 in c["counts"].tolist() and len(c["counts"]) == 3
    z1, tol1 = R.window_latents(c["content"], c["sums"], c["counts"], c["g_src"], c["g_trg"], 1.0, S)
    mean = c["sums"][:, :S] / c["counts"][:, None]
    assert np.array_equal(z1[:-1, :S], mean[c["g_trg"][:-1]])
    # g_src / g_trg swapped at mix = 1
    swapped, _ = R.window_latents(c["content"], c["sums"], c["counts"], c["g_trg"], c["g_src"], 1.0, S)
    assert not R.latents_close(swapped.astype(F32), z1, tol1)
    # the logvar half used for the style
    lv = np.concatenate([c["sums"][:, S:], c["sums"][:, :S]], axis=1)
    wrong, _ = R.window_latents(c["content"], lv, c["counts"], c["g_src"], c["g_trg"], 1.0, S)
    assert not R.latents_close(wrong.astype(F32), z1, tol1)
    # a padding window's row kept: counted into a group's style, or its latent row not zeroed
    kept = np.where(c["g_src"] < 0, 0, c["g_src"])
    sums_k, counts_k = R.group_sum(c["style"], kept, c["G"])
    for mix in (0.37, 1.0):
        z, tol = R.window_latents(c["content"], c["sums"], c["counts"], c["g_src"], c["g_trg"], mix, S)
        bad, _ = R.window_latents(c["content"], sums_k, counts_k, c["g_src"], c["g_trg"], mix, S)
        assert not R.latents_close(bad.astype(F32), z, tol)
    row, _ = R.window_latents(c["content"], c["sums"], c["counts"], kept, np.where(c["g_trg"] < 0, 1, c["g_trg"]), 1.0, S)
    assert not R.latents_close(row.astype(F32), z1, tol1)


def test_group_sum_restatement_is_sequential_and_skips_what_does_not_count():
    rows = np.asarray([[1, 2], [3, 4], [np.inf, 0], [5, 6]], F32)
    sums, counts = R.group_sum(rows, [0, 1, 0, -1], 2)
    assert sums.tolist() == [[1, 2], [3, 4]] and counts.tolist() == [1, 1]


def test_style_bank_is_data_only_and_round_trips(tmp_path):
    c = _convert()
    bank = c.StyleBank(["a", "b"], np.arange(16, dtype=F64).reshape(2, 8) / 7, [3, 1], 64, 32, 4, "DisentangledVAE_VCTK_5.pth")
    path = bank.save(tmp_path / "bank")
    assert path.endswith(".npz")
    with np.load(path, allow_pickle=False) as f:               # loads without pickle: data only
        assert sorted(f.files) == ["S", "T", "checkpoint", "counts", "hop", "names", "sums"]
    back = c.StyleBank.load(path)
    assert back.names == ["a", "b"] and (back.T, back.hop, back.S) == (64, 32, 4) and back.checkpoint == bank.checkpoint
    assert np.array_equal(back.sums.view(np.uint64), bank.sums.view(np.uint64)) and back.counts.tolist() == [3, 1]
    np.testing.assert_array_equal(back.mean("b"), bank.sums[1, :4] / 1)
    with pytest.raises(KeyError):
        back.index("c")
