"""Held-out validation on the MI355X: the two kernels of csrc/val.hip against the float64 restatement and the bounds of
tests/val_ref.py, `validate` on the smallest trainer shape the other trainer tests use (B = 4, T = 64), and the command line.

Measured on the MI355X with this file (worst error / bound): dvae_pair_metrics against float64 0.76 (n_per = 3), 0.34 on the
unaligned scalar path, 0.19 against dvae_loss_fwd; the group sums are bit-equal.  Every bound is the derived one of
tests/val_ref.py, none is fitted."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, child, DEV, dev_equal, down, EINVAL, F32, F64, guards, L, make_trainer, st
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib, data, ops  # noqa: E402
import elem_ref as E  # noqa: E402
import val_ref as V  # noqa: E402

SENT = -7.5e11


def guarded(data, dtype=torch.float32):
    """`data` in a guarded buffer whose payload lies 64 bytes behind a multiple of 256."""
    return Buf(dtype=dtype, data=np.asarray(data), lead=64)


def read(b):
    guards(b)
    return b.np()


def launch_pair(dev, out, Bh, n_per, D, S, mse, kl, shift=0):
    p = lambda k: dev[k].data_ptr() + (shift if k in ("x1", "x2", "rec", "rec_hat") else 0)
    return L().dvae_pair_metrics(*[p(k) for k in V.KEYS], out.ptr, Bh, n_per, D, S, mse, kl, st())


# ------------------------------------------------------------------ dvae_pair_metrics
@pytest.mark.parametrize("Bh", V.BH)
@pytest.mark.parametrize("n_per", V.N_PER)
def test_pair_metrics_against_float64_loss_fwd_and_itself(n_per, Bh):
    worst, worst_x = 0.0, 0.0
    for D in V.D:
        for S in V.S:
            d = V.pair_inputs(Bh, n_per, D, S, seed=1000 * Bh + n_per + D + S)
            dev = {k: torch.from_numpy(d[k]).to(DEV) for k in V.KEYS}
            mse, kl = 10.0, 3.0
            ref, tol = V.pair_bounds(*[d[k] for k in V.KEYS], mse, kl)
            outs = []
            for _ in range(2):
                out = guarded(np.full((Bh, 8), SENT, F32))
                assert launch_pair(dev, out, Bh, n_per, D, S, mse, kl) == 0
                outs.append(read(out))
            got = outs[0].astype(F64)
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))       # a second launch: the same bits
            r = float((np.abs(got - ref) / tol).max())
            worst = max(worst, r)
            assert r <= 1.0, (D, S, r, got, ref)
            if n_per % 4:
                continue
            # the existing kernel on the same tensors as one batch: out8 with scales (1 / Bh, -0.5 / Bh, -1 / Bh).  Both are
            # within their own bound of the same float64 number, except that dvae_loss_fwd multiplies by the fp32 value of
            # its scale (one rounding of 1 / Bh: eps32 relative) and forms out8[0] in fp32 from its own out8[1..6].
            ld = {"x1": d["x1"], "x2": d["x2"], "recon1": d["rec"][:Bh], "recon2": d["rec"][Bh:], "recon1_hat": d["rec_hat"][:Bh],
                  "recon2_hat": d["rec_hat"][Bh:], "q1_mu": d["q_mu"][:Bh], "q1_lv": d["q_lv"][:Bh], "q2_mu": d["q_mu"][Bh:],
                  "q2_lv": d["q_lv"][Bh:], "s_mu": d["s_mu"], "s_lv": d["s_lv"], "n": Bh * n_per, "nq": Bh * D, "ns": Bh * S,
                  "l1_scale": F32(1.0 / Bh), "kl_scale": F32(-0.5 / Bh), "style_scale": F32(-1.0 / Bh), "mse_cof": F32(mse),
                  "kl_cof": F32(kl)}
            desc = _lib.LossDesc()
            n = Bh * n_per
            for k, (t, lo) in {"x1": ("x1", 0), "x2": ("x2", 0), "recon1": ("rec", 0), "recon2": ("rec", n),
                               "recon1_hat": ("rec_hat", 0), "recon2_hat": ("rec_hat", n), "q1_mu": ("q_mu", 0),
                               "q1_lv": ("q_lv", 0), "q2_mu": ("q_mu", Bh * D), "q2_lv": ("q_lv", Bh * D), "s_mu": ("s_mu", 0),
                               "s_lv": ("s_lv", 0)}.items():
                setattr(desc, k, dev[t].data_ptr() + 4 * lo)
            desc.n, desc.nq, desc.ns = n, Bh * D, Bh * S
            for k in E.SCALE_KEYS:
                setattr(desc, k, float(ld[k]))
            out8 = guarded(np.full(8, SENT, F32))
            ws = torch.empty(L().dvae_loss_ws_bytes(n), dtype=torch.uint8, device=DEV)
            assert L().dvae_loss_fwd(ctypes.byref(desc), out8.ptr, ws.data_ptr(), st()) == 0
            o8 = read(out8).astype(F64)
            _, tol8 = E.loss_fwd_bounds(ld, o8)
            tol8[0] += mse * tol8[1:5].sum() + kl * (tol8[5] + tol8[6])         # out8[0] is bounded from the device's own parts
            both = tol8 + tol.mean(0) + 2 * V.EPS32 * np.abs(o8)                # + the rounding of the fp32 scale 1 / Bh
            rx = float((np.abs(got.mean(0) - o8) / both).max())
            worst_x = max(worst_x, rx)
            assert rx <= 1.0, (D, S, rx, got.mean(0), o8)
    print(f"n_per={n_per} Bh={Bh}: worst error / bound = {worst:.3f}; against dvae_loss_fwd {worst_x:.3f}")


def test_pair_metrics_unaligned_operands_take_the_scalar_path():
    """The same values 4 bytes further on: the scalar walk, to the same bound (its thread sums differ: not the same bits)."""
    Bh, n_per, D, S = 3, 1028, 32, 4
    d = V.pair_inputs(Bh, n_per, D, S, seed=77)
    dev = {}
    for k in V.KEYS:
        if k in ("x1", "x2", "rec", "rec_hat"):
            t = torch.zeros(d[k].size + 1, device=DEV)
            t[1:] = torch.from_numpy(d[k].reshape(-1))
            dev[k] = t
        else:
            dev[k] = torch.from_numpy(d[k]).to(DEV)
    ref, tol = V.pair_bounds(*[d[k] for k in V.KEYS], 10.0, 10.0)
    out = guarded(np.full((Bh, 8), SENT, F32))
    assert launch_pair(dev, out, Bh, n_per, D, S, 10.0, 10.0, shift=4) == 0
    r = float((np.abs(read(out).astype(F64) - ref) / tol).max())
    print(f"unaligned: worst error / bound = {r:.3f}")
    assert r <= 1.0


def test_pair_metrics_bad_arguments_write_nothing():
    Bh, n_per, D, S = 2, 8, 4, 2
    d = V.pair_inputs(Bh, n_per, D, S, seed=5)
    dev = {k: torch.from_numpy(d[k]).to(DEV) for k in V.KEYS}
    out = guarded(np.full((Bh, 8), SENT, F32))
    ptrs = [dev[k].data_ptr() for k in V.KEYS]
    for i in range(9):
        a = ptrs + [out.ptr]
        a[i] = None
        assert L().dvae_pair_metrics(*a, Bh, n_per, D, S, 10.0, 10.0, st()) == EINVAL, i
    for sizes in ((0, n_per, D, S), (-1, n_per, D, S), (Bh, 0, D, S), (Bh, -4, D, S), (Bh, n_per, 0, S), (Bh, n_per, D, 0)):
        assert L().dvae_pair_metrics(*ptrs, out.ptr, *sizes, 10.0, 10.0, st()) == EINVAL, sizes
    assert (read(out) == F32(SENT)).all()


# ------------------------------------------------------------------ dvae_group_sum_f64
class Sums:
    def __init__(self, G, K, old=None):
        rs = np.random.RandomState(G + K)
        self.G, self.K = G, K
        s0 = np.zeros((G + 1, K)) if old is None else rs.uniform(-1, 1, (G + 1, K))
        c0 = np.zeros(G + 1, np.int64) if old is None else rs.randint(0, 9, G + 1)
        b0 = np.zeros(G + 1, np.int64) if old is None else rs.randint(0, 9, G + 1)
        self.host = (s0, c0, b0)
        self.s, self.c, self.b = guarded(s0, torch.float64), guarded(c0, torch.int64), guarded(b0, torch.int64)

    def add(self, rows, group):
        r, g = torch.from_numpy(np.ascontiguousarray(rows, F32)).to(DEV), torch.from_numpy(np.asarray(group, np.int32)).to(DEV)
        assert L().dvae_group_sum_f64(r.data_ptr(), g.data_ptr(), rows.shape[0], self.K, self.G, self.s.ptr, self.c.ptr,
                                      self.b.ptr, st()) == 0
        self.host = V.group_sum(rows, group, self.G, *self.host)

    def check(self):
        s, c, b = read(self.s), read(self.c), read(self.b)
        assert np.array_equal(s.view(np.uint64), self.host[0].view(np.uint64)), "not the sequential float64 sum"
        assert np.array_equal(c, self.host[1]) and np.array_equal(b, self.host[2]), (c, b, self.host[1:])
        return s, c, b


def group_rows(P, G, K, seed):
    rs = np.random.RandomState(seed)
    rows = (rs.uniform(0, 1, (P, K)) * 10.0 ** rs.randint(-3, 4, (P, 1))).astype(F32)      # sums that do round
    return rows, rs.randint(0, G, P).astype(np.int32)


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("P", [1, 7, 300])
def test_group_sum_is_the_sequential_float64_sum(P, G):
    rows, group = group_rows(P, G, 8, 10 * P + G)
    for old in (None, True):                   # into zeroed buffers, and on top of what they held
        t = Sums(G, 8, old)
        t.add(rows, group)
        s, c, b = t.check()
        if old is None:
            assert c[G] == P and c[:G].sum() == P and not b.any()


def test_group_sum_three_calls_equal_one_on_the_concatenation():
    rows, group = group_rows(300 + 7 + 1, 5, 8, 3)
    one, three = Sums(5, 8), Sums(5, 8)
    one.add(rows, group)
    for lo, hi in ((0, 300), (300, 307), (307, 308)):
        three.add(rows[lo:hi], group[lo:hi])
    a, b = one.check(), three.check()
    assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


def test_group_sum_bad_rows_enter_no_sum():
    rows, group = group_rows(300, 5, 8, 4)
    rows[3, 2], rows[10, 7], rows[299, 0] = np.nan, np.inf, -np.inf
    group[20], group[21] = -1, 5
    t = Sums(5, 8)
    t.add(rows, group)
    s, c, b = t.check()
    assert np.isfinite(s).all() and c[5] == 295 and b[5] == 5
    assert b[:5].sum() == 3 and b[group[3]] >= 1 and c[:5].sum() == 295
    keep = np.ones(300, bool)
    keep[[3, 10, 299, 20, 21]] = False
    clean = V.group_sum(rows[keep], group[keep], 5)[0]
    assert np.array_equal(s.view(np.uint64), clean.view(np.uint64))


def test_group_sum_bad_arguments_write_nothing():
    rows, group = group_rows(7, 2, 8, 1)
    t = Sums(2, 8, old=True)
    r, g = torch.from_numpy(rows).to(DEV), torch.from_numpy(group).to(DEV)
    good = [r.data_ptr(), g.data_ptr(), 7, 8, 2, t.s.ptr, t.c.ptr, t.b.ptr]
    for i, v in ((0, None), (1, None), (5, None), (6, None), (7, None), (2, 0), (2, -1), (3, 0), (3, 257), (4, 0), (4, -2)):
        a = list(good)
        a[i] = v
        assert L().dvae_group_sum_f64(*a, st()) == EINVAL, (i, v)
    t.check()


# ------------------------------------------------------------------ validate on the trainer
B, T = 4, 64


class FixedPairs:
    """Seven pairs of two speakers with the interface of data.HeldOutPairs."""
    speaker_ids = ["a", "b", "c"]

    def __init__(self):
        from oracle.fill import synthetic_pair
        x1, x2 = synthetic_pair(7, T, 4242)
        self.x1, self.x2 = x1.cuda().float().contiguous(), x2.cuda().float().contiguous()
        self.spk = torch.tensor([0, 0, 2, 2, 2, 0, 2], dtype=torch.int32, device=DEV)

    def __len__(self):
        return 7

    def batches(self, bs):
        for lo in range(0, 7, bs):
            yield self.x1[lo:lo + bs], self.x2[lo:lo + bs], self.spk[lo:lo + bs]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """2 speakers x 12 utterances; 0.34 holds 4 files (2 pairs) of each out, 8 (4 pairs) train: two batches of 4 an epoch."""
    root = str(tmp_path_factory.mktemp("val_gpu") / "corpus")
    data.write_synthetic_corpus(root, n_speakers=2, n_utt=12, length=96, seed=0)
    held = data.split_corpus(root, 0.34, (), seed=0)
    assert sorted(len(v) for v in held.values()) == [4, 4]
    return {"root": root, "held": held, "ids": data.SpeechDatasetGVAE.list_speakers(root)}


def test_held_out_pairs_batches_are_the_centred_crops(corpus):
    hp = data.HeldOutPairs(corpus["held"], T, corpus["ids"], DEV)
    got = list(hp.batches(3))
    assert [b[0].shape[0] for b in got] == [3, 1] and len(hp) == 4              # a short last batch, no pair dropped
    x1, x2, spk = (torch.cat([b[i] for b in got]) for i in range(3))
    assert spk.dtype == torch.int32 and spk.is_cuda and spk.tolist() == [0, 0, 1, 1]
    for i, (a, b) in enumerate(hp.pairs):
        for x, f in ((x1, a), (x2, b)):
            assert np.array_equal(down(x[i]), np.load(f)[:, 16:16 + T].astype(F32)), (i, f)


@pytest.fixture(scope="module")
def trained(corpus, tmp_path_factory):
    """One trainer with the weight average and gradient clipping on, after one epoch of run_training (two steps of the
    command line's GPU loader on exclude=held, a checkpoint, validation of both weight sets), shared by the tests below."""
    out = tmp_path_factory.mktemp("val_trained")
    torch.cuda.manual_seed(11)
    w = make_trainer()
    w.optimizer.set_grad_clip(1e9)
    w.optimizer.set_ema(0.5)
    w.enable_graph(True)
    ds = data.SpeechDatasetGVAE(corpus["root"], samples_length=T, seed=3, exclude=corpus["held"])
    loader = data.GpuPairLoader(ds, B, device=DEV, seed=3)
    hp = data.HeldOutPairs(corpus["held"], T, corpus["ids"], DEV)
    hist = w.run_training(loader, None, 2, 2, reload_model=False, checkpoints_path=str(out / "checkpoints"),
                          logs_path=str(out / "logs"), logging_func=lambda *_: None, val_pairs=hp, val_interval=1)
    return {"w": w, "hist": hist, "out": out, "hp": hp, "loader": loader, "ds": ds}


def state_of(w, loader=None):
    opt = w.optimizer
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    s = {"flat_p": opt.flat_p.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
         "dev_state": opt.dev_state.clone(), "rng": torch.cuda.get_rng_state().clone(),
         "seed_offset": torch.tensor([gen.initial_seed(), gen.get_offset()])}
    for name in ("ema", "ema_state", "clip_state"):
        if getattr(opt, name, None) is not None:
            s[name] = getattr(opt, name).clone()
    for n, b in w.model.named_buffers():
        s["buf." + n] = b.clone()
    if loader is not None:
        for name, r in (("perm", loader.rng), ("crop", loader.crop_rng), ("pairs", loader.dataset.rng)):
            st_ = r.get_state()
            s["np." + name] = torch.from_numpy(np.concatenate([st_[1].astype(np.int64), [st_[2], st_[3]]]))
        s["pair_list"] = torch.tensor([hash(tuple(map(tuple, loader.dataset.utterance_fp))) & 0x7FFFFFFF])
    torch.cuda.synchronize()
    return s


def assert_same_state(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert dev_equal(a[k], b[k]), f"{what}: {k} changed"


VAL_KEYS = {"Val/" + t for t in dvae_amd.model.variational_base_vae.VariationalBaseModelVAE.VAL_TERMS} | \
    {"Val/Pairs", "Val/Non-finite pairs"}


def test_run_training_records_both_weight_sets_and_the_best_checkpoint(trained):
    hist, out = trained["hist"], trained["out"]
    assert [h["epoch"] for h in hist] == [1, 2]
    for h in hist:
        assert VAL_KEYS <= set(h) and {k.replace("Val/", "Val EMA/") for k in VAL_KEYS} <= set(h)
        assert h["Val/Pairs"] == h["Val EMA/Pairs"] == 4 and h["Val/Non-finite pairs"] == 0
        assert all(np.isfinite(v) for v in h.values())
    assert hist[0]["Val/Loss"] != hist[1]["Val/Loss"] and hist[1]["Val/Loss"] != hist[1]["Val EMA/Loss"]
    recs = [json.loads(line) for line in open(out / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert recs == hist
    val = json.load(open(out / "val.json"))
    assert val["epoch"] == 2 and set(val["per_speaker"]) == {"spk000", "spk001"} == set(val["per_speaker_ema"])
    per = val["per_speaker"]
    assert all(p["Pairs"] == 2 for p in per.values())
    assert abs(sum(p["Loss"] for p in per.values()) / 2 - hist[1]["Val/Loss"]) <= 1e-12 * hist[1]["Val/Loss"]
    best = json.load(open(out / "checkpoints" / "best.json"))
    lo, lo_ema = hist[1]["Val/Loss"], hist[1]["Val EMA/Loss"]
    assert best == {"epoch": 2, "weights": "DisentangledVAE_VCTK_2" + (".ema.pth" if lo_ema < lo else ".pth"),
                    "Val/Loss": min(lo, lo_ema), "ema": lo_ema < lo}
    assert (out / "checkpoints" / best["weights"]).is_file()


def test_validate_leaves_the_training_state_alone_and_repeats(trained):
    w, hp, loader = trained["w"], trained["hp"], trained["loader"]
    assert w.model.training
    before = state_of(w, loader)
    graph = w._graph
    a = w.validate(hp, lambda *_: None)
    a_ema = w.validate(hp, lambda *_: None, use_ema=True)
    assert_same_state(before, state_of(w, loader), "validate")
    assert w.model.training and w._graph is graph and not w.optimizer.ema_swapped
    b, b_ema = w.validate(hp, lambda *_: None), w.validate(hp, lambda *_: None, use_ema=True)
    assert a == b and a_ema == b_ema                                             # two passes: identical numbers
    assert {k: v for k, v in a.items() if k != "per_speaker"} == {k: v for k, v in trained["hist"][1].items() if k in VAL_KEYS}
    assert w.test(hp, 3, lambda *_: None) == a["Val/Loss"]
    w.model.eval()
    w.validate(hp, lambda *_: None)
    assert not w.model.training                                                  # restored, whichever it was
    w.model.train()


def test_validate_is_independent_of_the_batching(trained):
    """Seven pairs as 4 + 3, as one batch of 7, as 3 + 3 + 1, 5 + 2 and one at a time: the same per-pair rows bit for bit,
    totals within float64 rounding.  (Measured before `validate` fixed a pair's row in its launch: as 3 + 3 + 1 one of the 56
    values, pair 3's L1_2hat, was 2479.693603515625 against 2479.69384765625 — the H = 1024 recurrence adds its k-quarters in
    an order that turns with the row)"""
    w, fp = trained["w"], FixedPairs()
    res, rows = {}, {}
    for bs in (4, 7, 3, 5, 1):
        w.val_batch_size = bs
        try:
            res[bs] = w.validate(fp, lambda *_: None)
        finally:
            w.val_batch_size = None
        assert [r.shape[0] for r in w.val_rows] == [4, 3]                        # forwards of the trainer's B = 4, whatever came in
        rows[bs] = torch.cat(w.val_rows)
    for bs in (4, 3, 5, 1):
        a, b = down(rows[bs]), down(rows[7])
        where = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        print(f"batches of {bs} against one of 7: {len(where)} of {a.size} values differ in their bits",
              [(int(i), int(j), float(a[i, j]), float(b[i, j])) for i, j in where])
    for bs in (4, 3, 5, 1):
        assert dev_equal(rows[bs], rows[7]), bs
        for k in VAL_KEYS:
            assert abs(res[bs][k] - res[7][k]) <= 16 * V.EPS64 * abs(res[7][k]), (bs, k)
    assert res[4]["Val/Pairs"] == 7 and set(res[4]["per_speaker"]) == {"a", "c"}
    assert res[4]["per_speaker"]["a"]["Pairs"] == 3 and res[4]["per_speaker"]["c"]["Pairs"] == 4
    total = down(rows[7]).astype(F64)
    seq = V.group_sum(down(rows[7]), down(fp.spk), 3)[0]
    assert res[7]["Val/Loss"] == seq[3, 0] / 7 and abs(res[7]["Val/Loss"] - total[:, 0].mean()) <= 16 * V.EPS64 * total[:, 0].mean()


def test_val_ema_numbers_are_those_of_the_averaged_checkpoint(trained):
    w, hp, out = trained["w"], trained["hp"], trained["out"]
    p_before = w.optimizer.flat_p.clone()
    got = w.validate(hp, lambda *_: None, use_ema=True)
    assert dev_equal(w.optimizer.flat_p, p_before)                               # the live weights are back
    assert got == {k: v for k, v in got.items()} and got["Val EMA/Loss"] == trained["hist"][1]["Val EMA/Loss"]
    c = make_trainer()
    c.model.load_state_dict(torch.load(out / "checkpoints" / "DisentangledVAE_VCTK_2.ema.pth", map_location="cuda"))
    ref = c.validate(hp, lambda *_: None)
    del c
    for t in w.VAL_TERMS:
        assert got["Val EMA/" + t] == ref["Val/" + t], t
    assert got["per_speaker"] == ref["per_speaker"]
    live = w.validate(hp, lambda *_: None)
    assert live["Val/Loss"] != got["Val EMA/Loss"]


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_a_run_that_validates_trains_exactly_as_one_that_does_not(corpus, graph):
    """Run A validates after each of its two epochs, run B never does: weights, moments, BatchNorm buffers and the default
    generator end bit-identical — a pass between two replays of the captured step changes neither."""
    ends = []
    for validates in (True, False):
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        w = make_trainer()
        w.enable_graph(graph)
        ds = data.SpeechDatasetGVAE(corpus["root"], samples_length=T, seed=9, exclude=corpus["held"])
        loader = data.GpuPairLoader(ds, B, device=DEV, seed=9)
        kw = {"val_pairs": data.HeldOutPairs(corpus["held"], T, corpus["ids"], DEV)} if validates else {}
        hist = w.run_training(loader, None, 2, 5, reload_model=False, logging_func=lambda *_: None, **kw)
        assert ("Val/Loss" in hist[1]) == validates and len(loader) == 2
        assert (w._graph is not None) == graph
        ends.append((state_of(w, loader), [{k: v for k, v in h.items() if not k.startswith("Val")} for h in hist]))
        del w
    assert_same_state(ends[0][0], ends[1][0], "a validating run")
    assert ends[0][1] == ends[1][1]


# ------------------------------------------------------------------ the command line
@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """Two training runs of the command line on one synthetic corpus: two epochs with --val-fraction 0.25 --ema-decay 0.9
    (4 of 16 files of either speaker held out: 4 validation pairs, 12 training pairs, three steps an epoch), and one with
    none of the new flags."""
    root = tmp_path_factory.mktemp("val_cli")
    corpus = data.write_synthetic_corpus(str(root / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)
    common = [f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4", "--epochs=2",
              "--report-interval=2", "--mse_cof=10", "--kl_cof=10", "--seed=3", "--src_spk=spk000", "--trg_spk=spk001",
              "--convert-count=1", "--griffin-lim-iters=2"]
    out = {"corpus": corpus, "common": common}
    for name, extra in (("val", ["--val-fraction", "0.25", "--ema-decay", "0.9"]), ("plain", [])):
        out[name] = root / name
        child("train", ["--train", "true", "--do-not-resume", f"--log_dir={out[name]}"] + common + extra)
    return out


def test_train_cli_validates_and_convert_follows_best_json(cli_runs):
    log = cli_runs["val"]
    recs = [json.loads(line) for line in open(log / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert [r["epoch"] for r in recs] == [1, 2]
    for r in recs:
        assert VAL_KEYS <= set(r) and {k.replace("Val/", "Val EMA/") for k in VAL_KEYS} <= set(r), sorted(r)
        assert r["Val/Pairs"] == 4 and r["Val/Non-finite pairs"] == 0 and all(np.isfinite(v) for v in r.values())
    split = json.load(open(log / "val_split.json"))
    assert split["val_fraction"] == 0.25 and split["val_speakers"] == [] and split["val_seed"] == 0
    assert {k: len(v) for k, v in split["held_out"].items()} == {"spk000": 4, "spk001": 4}
    assert set(json.load(open(log / "val.json"))["per_speaker"]) == {"spk000", "spk001"}
    best = json.load(open(log / "checkpoints" / "best.json"))
    assert best["epoch"] == 2 and (log / "checkpoints" / best["weights"]).is_file()
    assert best["Val/Loss"] == min(recs[1]["Val/Loss"], recs[1]["Val EMA/Loss"])
    child("train", ["--convert", "true", "--use-best", f"--log_dir={log}"] + cli_runs["common"])
    wav = log / "generation" / "spk000_to_spk001" / "convert_spk000_to_spk001_utt000.wav"
    assert wav.is_file() and wav.stat().st_size > 44


def test_resume_with_another_split_exits(cli_runs):
    r = child("train", ["--train", "true", f"--log_dir={cli_runs['val']}", "--val-fraction", "0.4", "--ema-decay", "0.9"]
               + cli_runs["common"], ok=False)
    assert r.returncode != 0 and "val_split.json" in r.stderr and "val_fraction" in r.stderr and "leak" in r.stderr, \
        (r.returncode, r.stderr[-2000:])
    assert sorted(f for f in os.listdir(cli_runs["val"] / "checkpoints") if f.endswith(".pth")) == \
        ["DisentangledVAE_VCTK_2.ema.pth", "DisentangledVAE_VCTK_2.pth"]          # nothing was trained


def test_run_without_the_flags_is_what_it_was(cli_runs):
    log = cli_runs["plain"]
    recs = [json.loads(line) for line in open(log / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert [r["epoch"] for r in recs] == [1, 2] and not any(k.startswith("Val") for r in recs for k in r)
    assert not {"val_split.json", "val.json"} & set(os.listdir(log))
    assert sorted(os.listdir(log / "checkpoints")) == ["DisentangledVAE_VCTK_2.opt", "DisentangledVAE_VCTK_2.pth"]
    assert not any(k.startswith("val") or k == "use_best" for k in json.load(open(log / "config.json")))
    r = child("train", ["--convert", "true", "--use-best", f"--log_dir={log}"] + cli_runs["common"], ok=False)
    assert r.returncode != 0 and "best.json" in r.stderr
