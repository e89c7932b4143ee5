"""CPU checks of held-out validation: the float64 restatement of csrc/val.hip (tests/val_ref.py) against the oracle's
loss_functionGVAE2, the split of the corpus, `exclude=`, the fixed pair list, val_split.json and best.json.  No GPU: the
kernels are held to the restatement in tests/test_hip_val.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from dvae_amd import data  # noqa: E402
import val_ref as V  # noqa: E402


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("Bh,n_per,D,S", [(1, 1, 1, 1), (3, 1028, 32, 4), (4, 5120, 257, 4)])
def test_mean_of_the_rows_is_the_oracle_loss_of_a_full_batch(Bh, n_per, D, S):
    from oracle.dvae_ref import loss_gvae2
    d = V.pair_inputs(Bh, n_per, D, S, seed=Bh + n_per)
    rows = V.pair_rows(*[d[k] for k in V.KEYS], 10.0, 3.0)
    t = {k: torch.from_numpy(d[k].astype(np.float64)) for k in V.KEYS}
    outs = (t["rec"][:Bh], t["rec"][Bh:], t["rec_hat"][:Bh], t["rec_hat"][Bh:], t["q_mu"][:Bh], t["q_lv"][:Bh],
            t["q_mu"][Bh:], t["q_lv"][Bh:], t["s_mu"], t["s_lv"])
    ref = np.array([float(v) for v in loss_gvae2(t["x1"], t["x2"], outs, Bh, 10.0, 3.0)])
    got = rows.mean(0)
    # float64 rounding: both are sums of the same n terms; the cancelling KL sums against their absolute terms
    scale = np.abs(ref).copy()
    scale[5:] = np.maximum(scale[5:], (1.0 + np.abs(d["q_lv"]).max() + (d["q_mu"].astype(np.float64) ** 2).max() + np.e ** 2) * D)
    scale[0] = 10.0 * scale[1:5].sum() + 3.0 * (scale[5] + scale[6])
    assert np.all(np.abs(got - ref) <= 64 * V.EPS64 * scale), (got, ref)
    assert rows.shape == (Bh, 8) and np.all(rows[:, 1:] >= 0) and np.all(rows[:, 0] > 0)


def test_bounds_are_small_positive_and_the_cases_reach_every_path():
    d = V.pair_inputs(3, 5120, 32, 4, seed=1)
    ref, tol = V.pair_bounds(*[d[k] for k in V.KEYS], 10.0, 10.0)
    assert np.all(tol > 0) and np.all(tol[:, 1:5] <= 3 * V.EPS32 * ref[:, 1:5])         # two roundings and dust
    assert np.all(tol[:, 5:] < 1e-4) and np.all(tol[:, 0] <= 10 * tol[:, 1:5].sum(1) + 10 * (tol[:, 5] + tol[:, 6]) + 1e-9)
    assert [V.uses_float4(n) for n in V.N_PER] == [False, False, True, True, True, True, True]
    assert [V.thread_trips(n) for n in V.N_PER] == [1, 1, 1, 1, 1, 2, 5]                  # 1024 / 4 = 256: the last full trip
    assert not V.uses_float4(1024, aligned=False) and V.thread_trips(1024, aligned=False) == 4
    assert 1 in V.D and max(V.D) > V.WG and 1 in V.S


def test_group_sum_restatement():
    rows = np.arange(40, dtype=np.float32).reshape(5, 8)
    rows[3, 2] = np.inf
    s, c, b = V.group_sum(rows, [0, 1, 1, 1, 7], 2)
    assert np.array_equal(s[0], rows[0]) and np.array_equal(s[1], rows[1].astype(np.float64) + rows[2])
    assert np.array_equal(s[2], s[0] + s[1]) and list(c) == [1, 2, 3] and list(b) == [0, 1, 2]
    s2, c2, b2 = V.group_sum(rows[:1], [1], 2, s, c, b)
    assert np.array_equal(s2[1], s[1] + rows[0]) and list(c2) == [1, 3, 4] and list(b2) == list(b)


# ------------------------------------------------------------------ the split
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = tmp_path_factory.mktemp("val_corpus")
    data.write_synthetic_corpus(str(root), n_speakers=3, n_utt=11, length=96, seed=0)
    for u in range(11):                     # a speaker of short utterances: zero padding instead of a crop
        np.save(root / "spk002" / f"utt{u:03d}_mel.npy", np.random.RandomState(u).uniform(0, 1, (80, 40)))
    return str(root)


def test_split_is_deterministic_even_and_per_speaker(corpus):
    a = data.split_corpus(corpus, 0.3, (), seed=0)
    assert a == data.split_corpus(corpus, 0.3, (), seed=0)
    assert sorted(a) == ["spk000", "spk001", "spk002"]
    for spk, files in a.items():
        assert len(files) == 2 == (int(0.3 * 11) & ~1) and files == sorted(files)
        assert all(os.path.basename(os.path.dirname(f)) == spk and os.path.exists(f) for f in files)
    assert a != data.split_corpus(corpus, 0.3, (), seed=1)                    # the seed moves it
    names = lambda h: [os.path.basename(f) for f in h]
    assert names(a["spk000"]) != names(a["spk001"]) or names(a["spk001"]) != names(a["spk002"])      # not one rule for all
    assert data.split_corpus(corpus, 0.0) == {} and data.split_corpus(corpus, 0.1) == {}              # floor(1.1) -> 0
    assert all(len(v) == 4 for v in data.split_corpus(corpus, 0.49).values())                         # floor(5.39) = 5 -> 4
    for bad in (-0.1, 0.5, 0.9):
        with pytest.raises(ValueError, match="val_fraction"):
            data.split_corpus(corpus, bad)


def test_split_does_not_depend_on_the_listing_order(corpus, monkeypatch):
    want = data.split_corpus(corpus, 0.4, ("spk001",), seed=5)
    real_listdir, real_glob = os.listdir, data.glob.glob
    monkeypatch.setattr(data.os, "listdir", lambda p: list(reversed(sorted(real_listdir(p)))))
    monkeypatch.setattr(data.glob, "glob", lambda p: list(reversed(sorted(real_glob(p)))))
    assert data.split_corpus(corpus, 0.4, ("spk001",), seed=5) == want


def test_val_speakers_are_held_out_whole_and_unknown_ones_raise(corpus):
    h = data.split_corpus(corpus, 0.0, ("spk001",))
    assert list(h) == ["spk001"] and len(h["spk001"]) == 10                   # 11 files: the odd last one is dropped ...
    ex = data.excluded_files(corpus, 0.0, ("spk001",))
    assert len(ex) == 11 and set(h["spk001"]) < set(ex)                       # ... and not trained on either
    ds = data.SpeechDatasetGVAE(corpus, seed=0, exclude=ex)
    assert ds.speaker_ids == ["spk000", "spk001", "spk002"] and [len(u) for u in ds.spk_utt] == [11, 0, 11]
    with pytest.raises(ValueError, match="nobody"):
        data.split_corpus(corpus, 0.2, ("nobody",))


def test_exclude_keeps_held_out_files_out_of_five_epochs(corpus):
    held = data.split_corpus(corpus, 0.4, (), seed=2)
    out = {f for fs in held.values() for f in fs}
    assert len(out) == 12
    ds = data.SpeechDatasetGVAE(corpus, seed=3, exclude=held)
    seen = set()
    for _ in range(5):
        assert len(ds) == 9                                                    # 7 files left per speaker: 3 pairs each
        seen |= {f for pair in ds.utterance_fp for f in pair}
        labels = {ds[i][2].item() for i in range(len(ds))}
        assert labels == {0, 1, 2}                                             # the labels of the whole listing
        ds.shuffle_data()
    assert not seen & out and len(seen) > 12


def test_exclude_none_is_the_dataset_of_today(corpus):
    a, b = data.SpeechDatasetGVAE(corpus, seed=7), data.SpeechDatasetGVAE(corpus, seed=7, exclude=None)
    for _ in range(2):
        assert np.array_equal(a.utterance_fp, b.utterance_fp)
        a.shuffle_data()
        b.shuffle_data()
    assert a.speaker_ids == b.speaker_ids
    # the pair list a seeded dataset gave before `exclude` existed: shuffle, halves, i-th with i-th
    rng, pairs = np.random.RandomState(7), []
    for s in a.speaker_ids:
        utt = np.array(sorted(data.glob.glob(os.path.join(corpus, s, "*.npy"))))
        rng.shuffle(utt)
        pairs += [(utt[i], utt[len(utt) // 2 + i]) for i in range(len(utt) // 2)]
    assert np.array_equal(data.SpeechDatasetGVAE(corpus, seed=7).utterance_fp, np.array(pairs, dtype=object).reshape(-1, 2))


def test_held_out_pairs_list_and_centred_offsets(corpus):
    held = data.split_corpus(corpus, 0.4, (), seed=2)
    ids = data.SpeechDatasetGVAE.list_speakers(corpus)
    hp = data.HeldOutPairs(held, 64, ids, device=None)
    assert len(hp) == 6 and list(hp.speakers) == [0, 0, 1, 1, 2, 2]
    want = []
    for s in ids:
        f = sorted(held[s])
        want += [(f[0], f[2]), (f[1], f[3])]                                   # file i with file k/2 + i, sorted order
    assert hp.pairs == want
    again = data.HeldOutPairs(held, 64, ids, device=None)
    assert again.pairs == hp.pairs and np.array_equal(again.offsets, hp.offsets)      # no shuffling, ever
    for f, i in hp.index.items():
        L = np.load(f).shape[1]
        assert hp.lengths[i] == L and L in (96, 40)
        assert hp.offsets[i] == ((96 - 64) // 2 if L == 96 else 0)             # centred crop; short: start 0, zeros behind
    assert {int(hp.lengths[i]) for i in hp.u1[4:]} == {40} and {int(hp.lengths[i]) for i in hp.u1[:4]} == {96}
    with pytest.raises(RuntimeError, match="pair list only"):
        next(hp.batches(4))


# ------------------------------------------------------------------ the files
def test_val_split_json_round_trip_and_mismatch_exits(corpus, tmp_path):
    held = data.split_corpus(corpus, 0.3, ("spk002",), seed=4)
    ex = data.excluded_files(corpus, 0.3, ("spk002",), seed=4)
    path = str(tmp_path / "val_split.json")
    data.write_val_split(path, corpus, held, ex, 0.3, ("spk002",), 4)
    rec = json.load(open(path))
    assert rec["val_fraction"] == 0.3 and rec["val_speakers"] == ["spk002"] and rec["val_seed"] == 4
    assert all(not os.path.isabs(f) and "\\" not in f for fs in rec["held_out"].values() for f in fs)
    h2, e2 = data.read_val_split(path, corpus, 0.3, ("spk002",), 4)
    assert h2 == held and sorted(e2) == sorted(ex)
    for args, word in (((0.2, ("spk002",), 4), "val_fraction"), ((0.3, (), 4), "val_speakers"), ((0.3, ("spk002",), 5), "val_seed"),
                       ((0.0, (), 0), "val_fraction")):
        with pytest.raises(SystemExit, match=word) as e:
            data.read_val_split(path, corpus, *args)
        assert "leak" in str(e.value)


def test_train_cli_reads_the_split_of_the_first_run(corpus, tmp_path):
    from dvae_amd import train
    argv = [f"--dataset_fp={corpus}", f"--log_dir={tmp_path}", "--val-fraction", "0.3"]
    args = train.get_parse().parse_args(argv)
    held, ex = train.held_out_split(args)
    assert held == data.split_corpus(corpus, 0.3) and os.path.exists(tmp_path / "val_split.json")
    assert train.held_out_split(args) == (held, ex)                            # a resumed run: read back
    with pytest.raises(SystemExit, match="val_fraction"):
        train.held_out_split(train.get_parse().parse_args(argv[:2] + ["--val-fraction", "0.4"]))
    with pytest.raises(SystemExit, match="val_fraction"):
        train.held_out_split(train.get_parse().parse_args(argv[:2]))            # the flags dropped: a leak as well
    none = train.get_parse().parse_args([f"--dataset_fp={corpus}", f"--log_dir={tmp_path / 'other'}"])
    assert train.held_out_split(none) == (None, None) and not (tmp_path / "other").exists()
    with pytest.raises(SystemExit, match="best.json"):
        train.load_best(None, str(tmp_path))


def test_best_json_is_invisible_to_checkpoint_discovery(tmp_path):
    from dvae_amd.model.variational_base_vae import VariationalBaseModelVAE

    class Named(torch.nn.Module):
        pass

    w = VariationalBaseModelVAE(None, 64, 80, 1, 32, 1e-3, "cpu", 500, 4)
    w.model = Named()
    (tmp_path / "best.json").write_text(json.dumps({"epoch": 3, "weights": "DisentangledVAE_VCTK_3.pth", "Val/Loss": 1.0,
                                                    "ema": False}))
    said = []
    assert w.load_last_model(str(tmp_path), said.append) == 1 and "from scratch" in said[0]
    # and the rule of the trainer's best.json: the lowest Val/Loss of any checkpoint, an existing file counts
    val = lambda a, b: {"last": {"Val/Loss": a}, "ema": {"Val EMA/Loss": b}}
    for e in (4, 5, 6):
        (tmp_path / f"DisentangledVAE_VCTK_{e}.pth").write_bytes(b"")
    (tmp_path / "DisentangledVAE_VCTK_5.ema.pth").write_bytes(b"")
    os.remove(tmp_path / "best.json")
    w._note_best(str(tmp_path), "DisentangledVAE_VCTK_4", 4, val(2.0, 1.0))    # no .ema.pth written: not a candidate
    assert json.load(open(tmp_path / "best.json")) == {"epoch": 4, "weights": "DisentangledVAE_VCTK_4.pth", "Val/Loss": 2.0,
                                                       "ema": False}
    w._note_best(str(tmp_path), "DisentangledVAE_VCTK_5", 5, val(1.9, 1.5))
    assert json.load(open(tmp_path / "best.json")) == {"epoch": 5, "weights": "DisentangledVAE_VCTK_5.ema.pth", "Val/Loss": 1.5,
                                                       "ema": True}
    w._note_best(str(tmp_path), "DisentangledVAE_VCTK_6", 6, val(1.7, float("nan")))
    assert json.load(open(tmp_path / "best.json"))["epoch"] == 5                # not lower: the pointer stays
    names = [f for f in os.listdir(tmp_path) if f.endswith(".pth")]
    assert "best.json" in os.listdir(tmp_path) and all(not f.startswith("best") for f in names)
