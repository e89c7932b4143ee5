"""The speaker adversary on the training step (ConvolutionalMulVAE.set_speaker_adversary) on the MI355X:
with weight 0 the model's step keeps its bits while the classifier learns, a warm-up changes the weight every step under ONE
captured graph that equals the eager step bit for bit, switching it off restores the old graph signature, what cannot work is
refused, ops.SpeakerAdversaryFn stays inside the restatement's bounds, and the command line writes, resumes and refuses."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import child, dev_equal, make_trainer
import adv_ref as A  # noqa: E402
from ref_common import worst_ratio  # noqa: E402

B, T, SPK = 4, 64, 5
MODEL_BUFS = ("flat_p", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def feed():
    from oracle.fill import synthetic_eps, synthetic_pair
    data = [tuple(t.cuda() for t in synthetic_pair(B, T, 700 + i)) for i in range(3)]
    noise = [synthetic_eps(B, seed=800 + i) for i in range(3)]
    gen = torch.Generator().manual_seed(5)
    ids = [torch.randint(0, SPK, (B,), generator=gen) for _ in range(3)]
    return data, noise, ids


def run(w, feed, steps, ids=True, after=None):
    data, noise, spk = feed
    out, extra = [], []
    for i in range(steps):
        w.model.eps_override = noise[(2 * i) % 3]
        out.append(w.step(*data[i % 3], spk[i % 3] if ids else None, train=True))
        if after is not None:
            extra.append(after(i))
    return out, extra


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_weight_zero_leaves_the_model_its_bits(feed, graph):
    a, b = make_trainer(B, T), make_trainer(B, T)
    b.set_speaker_adversary(0.0, n_speakers=SPK)
    before = b.adversary.optimizer.flat_p.clone()
    for w in (a, b):
        w.enable_graph(graph)
    la, _ = run(a, feed, 6, ids=False)
    lb, ces = run(b, feed, 6, after=lambda i: b.adv_out.tolist())
    assert la == lb
    for name in MODEL_BUFS:
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    adv = b.adversary
    assert not dev_equal(adv.optimizer.flat_p, before) and adv.optimizer.t == 6 and b.optimizer.t == 6
    assert all(math.isfinite(v) for c in ces for v in c) and all(c[1] == 2 * B for c in ces)
    assert b._adv_coef.tolist() == [0.0]
    # the padding of the classifier's parameters is zero and stays zero
    assert not adv.params["b2"][SPK:].any() and not adv.params["w1"][:, adv.dim:].any()
    assert adv.optimizer._zero_ranges == [] and adv.optimizer.numel == adv.optimizer.n_used


def test_warmup_under_one_graph_equals_eager(feed):
    a, b, z = make_trainer(B, T), make_trainer(B, T), make_trainer(B, T)
    for w in (a, b):
        w.set_speaker_adversary(0.5, n_speakers=SPK, warmup_steps=5)
    z.set_speaker_adversary(0.0, n_speakers=SPK)
    b.enable_graph(True)
    graphs = []
    la, ca = run(a, feed, 8, after=lambda i: a._adv_coef.tolist()[0])
    lb, cb = run(b, feed, 8, after=lambda i: (graphs.append(b._graph), b._adv_coef.tolist()[0])[1])
    lz, _ = run(z, feed, 8)
    assert la == lb
    for name in MODEL_BUFS:
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
        assert dev_equal(getattr(a.adversary.optimizer, name), getattr(b.adversary.optimizer, name)), "adversary " + name
    assert dev_equal(a.adv_out, b.adv_out) and dev_equal(a.adv_pred, b.adv_pred)
    # one capture (at the second step), replayed to the end although the weight took six values
    assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])
    want = [float(np.float32(0.5 * min(1.0, k / 5))) for k in range(8)]
    assert ca == want and cb == want and len(set(want)) == 6
    assert a._step_k == b._step_k == 8 and a.adversary.optimizer.t == 8
    # the first step ran under weight 0: the model's loss vector is the monitor's; later the encoder has been pushed
    assert la[0] == lz[0] and la[1] == lz[1]          # (step 1's weights moved under lambda = 0 as well)
    assert any(u != v for u, v in zip(la[2:], lz[2:]))
    assert not dev_equal(a.optimizer.flat_p, z.optimizer.flat_p)


def test_none_restores_the_old_graph_signature(feed):
    data, _, _ = feed
    w = make_trainer(B, T)
    plain = w._graph_signature(data[0][0])
    w.set_speaker_adversary(0.25, n_speakers=SPK, hidden=128)
    assert w._graph_signature(data[0][0]) == plain + (("adv", 128, SPK),)
    w.enable_graph(True)
    run(w, feed, 3)
    with_adv = w._graph
    assert with_adv is not None
    w.set_speaker_adversary(None)
    assert w.adversary is None and w._graph_signature(data[0][0]) == plain
    run(w, feed, 2, ids=False)                        # no labels needed any more; captured again without the two launches
    assert w._graph is not None and w._graph is not with_adv


def test_refusals(feed):
    data, noise, _ = feed
    w = make_trainer(B, T)
    w.set_speaker_adversary(0.5, n_speakers=SPK)
    w.model.eps_override = noise[0]
    for graph in (False, True):
        w.enable_graph(graph)
        with pytest.raises(ValueError, match="speaker_ids"):
            w.step(*data[0], None, train=True)
    with pytest.raises(ValueError, match="data parallel"):
        w.attach_reducer(object())
    assert w.reducer is None
    r = make_trainer(B, T)
    r.reducer = object()
    with pytest.raises(ValueError, match="data parallel"):
        r.set_speaker_adversary(0.5, n_speakers=SPK)
    assert getattr(r, "adversary", None) is None
    r.reducer = None
    for bad in (dict(weight=-0.1, n_speakers=SPK), dict(weight=0.5), dict(weight=0.5, n_speakers=SPK, hidden=100),
                dict(weight=0.5, n_speakers=2000), dict(weight=0.5, n_speakers=SPK, warmup_steps=-1)):
        with pytest.raises(ValueError):
            r.set_speaker_adversary(bad.pop("weight"), **bad)


def test_function_on_a_leaf_q_mu():
    """ops.SpeakerAdversaryFn on the training step's shape: the columns 4 .. 31 of a leaf [128, 32], against the restatement"""
    from dvae_amd import ops
    from dvae_amd.adversary import SpeakerAdversary
    c = A.make_case("step")
    R, D, H, S = c["R"], c["D"], c["H"], c["S"]
    adv = SpeakerAdversary(D, S, hidden=H, seed=3)
    with torch.no_grad():
        for k in ("w1", "b1", "w2", "b2"):
            p = adv.params[k]
            p.zero_()
            src = torch.from_numpy(np.asarray(c[k]))
            p[tuple(slice(0, n) for n in src.shape)] = src.cuda()
    table = torch.randn(R, 4 + D, device="cuda")
    table[:, 4:] = torch.from_numpy(c["x"]).cuda()
    q = table.clone().requires_grad_(True)
    labels = torch.from_numpy(c["labels"]).cuda()
    coef = torch.tensor([c["lam"]], device="cuda")
    stats = {}
    ce = adv.loss(q, labels, coef, 4, stats)
    with pytest.raises(RuntimeError, match="unit_seed"):
        ce.backward(retain_graph=True)                   # autograd's own ones: any seed but THE one is refused
    with pytest.raises(RuntimeError, match="unit_seed"):
        torch.autograd.backward([2.0 * ce], [ops.unit_seed(q.device)], retain_graph=True)
    assert q.grad is None
    torch.autograd.backward([ce], [ops.unit_seed(q.device)])
    args = (c["x"], c["labels"], c["w1"], c["b1"], c["w2"], c["b2"], c["lam"], c["inv_rows"])
    res = A.rows64(*args)
    par, bnd = A.params64(c["x"], c["labels"], res, c["inv_rows"]), A.bounds(*args, res=res)
    g = q.grad.cpu().numpy()
    assert not g[:, :4].any()
    got = {"dx": g[:, 4:], "dw1": adv.params["w1"].grad[:, :D].cpu().numpy(), "db1": adv.params["b1"].grad.cpu().numpy(),
           "dw2": adv.params["w2"].grad.cpu().numpy(), "db2": adv.params["b2"].grad[:S].cpu().numpy()}
    ref = dict(par, dx=res["dx"])
    for k, v in got.items():
        r, i = worst_ratio(v, ref[k], bnd[k])
        assert r <= 1.0, (k, r, i)
    assert worst_ratio([ce.item()], [par["out"][3]], [bnd["out"][3]])[0] <= 1.0
    assert stats["out"].tolist()[1:3] == list(par["out"][1:3]) and np.array_equal(stats["row_pred"].cpu().numpy(), res["pred"])
    assert not adv.params["b2"].grad[S:].any() and not adv.params["w1"].grad[:, D:].any()
    ev = adv.evaluate(torch.from_numpy(c["x"]), c["labels"])
    assert ev["n"] == R and math.isclose(ev["loss"], par["out"][0] / R, rel_tol=1e-5) and ev["accuracy"] == par["out"][2] / R
    # state: parameters, moments, step count, configuration
    adv.optimizer.step()
    sd = adv.state_dict()
    other = SpeakerAdversary(D, S, hidden=H, seed=9)
    with pytest.raises(ValueError):
        other.load_state_dict(sd)
    same = SpeakerAdversary(D, S, hidden=H, seed=3)
    same.load_state_dict(sd)
    assert same.optimizer.t == 1
    for name in MODEL_BUFS:
        assert dev_equal(getattr(same.optimizer, name), getattr(adv.optimizer, name)), name


def test_the_reversal_pushes_the_encoder_against_the_classifier(feed):
    """the sign at the trainer's level: after ONE step on a batch, a FROZEN copy of the initial classifier finds the content means
    of the model stepped under a weight so large that the reversed gradient decides the sign of every encoder gradient it
    reaches harder (a higher cross-entropy) than those of the model stepped under weight 0.  To first order the difference is
    (lr / weight) sum_i g_adv,i (sign(g_loss,i + g_adv,i) - sign(g_loss,i)) >= 0 under Adam's first, sign-like step, and far
    from 0 once g_adv dominates.  (At weights near 1 the reversed gradient is orders of magnitude below the reconstruction
    loss's, mse_cof times an L1 SUM over the mel: 20 was tried and the difference drowned, -0.002, in three steps' noise.)"""
    from dvae_amd.adversary import SpeakerAdversary
    data, noise, ids = feed
    labels = torch.cat([ids[0], ids[0]])
    ce = {}
    for lam in (0.0, 1e6):
        w = make_trainer(B, T)
        w.set_speaker_adversary(lam, n_speakers=SPK)
        S = w.model.speaker_size
        frozen = SpeakerAdversary(w.model.latent_dim - S, SPK, seed=0)          # the trainer's classifier as it started
        assert dev_equal(frozen.optimizer.flat_p, w.adversary.optimizer.flat_p)
        w.model.eps_override = noise[0]
        w.step(*data[0], ids[0], train=True)
        with torch.no_grad():
            q_mu = w.model.forward_full(*data[0])[2]
        ce[lam] = frozen.evaluate(q_mu[:, S:].contiguous(), labels)["loss"]
    print("cross-entropy under the frozen classifier:", ce)
    assert ce[1e6] > ce[0.0] + 1e-4, ce


def test_estimation_at_a_checkpoint_leaves_the_noise_generator_alone(feed, tmp_path):
    """no adversary: estimate_trained_model draws the style noise of its eval-mode forward and puts the default generator back,
    so the step behind a checkpoint draws what a run resumed from it draws"""
    data, _, ids = feed
    w = make_trainer(B, T)
    ck = tmp_path / "ck"
    ck.mkdir()
    torch.save(w.model.state_dict(), str(ck / "DisentangledVAE_VCTK_1.pth"))
    torch.cuda.manual_seed(77)
    before = torch.cuda.get_rng_state()
    loader = [(data[0][0].cpu(), data[0][1].cpu(), ids[0])]
    epoch, r1, _ = w.estimate_trained_model(loader, str(ck), str(tmp_path / "est"))
    assert epoch == 2 and torch.equal(torch.cuda.get_rng_state(), before)
    again = w.estimate_trained_model(loader, str(ck), str(tmp_path / "est"))[1]
    assert dev_equal(r1, again)                           # the same noise both times: the draw does happen, from `before`
    assert not torch.equal(torch.randn(4, device="cuda"), torch.zeros(4, device="cuda")) and \
        not torch.equal(torch.cuda.get_rng_state(), before)


def test_inference_callers_load_an_adversary_run_like_any_other(feed, tmp_path):
    """load_last_model restores the adversary only for run_training; a trainer that asked for one still gets the checks"""
    w = make_trainer(B, T)
    w.set_speaker_adversary(0.5, n_speakers=SPK, hidden=64)
    run(w, feed, 1)
    ck = tmp_path / "ck"
    ck.mkdir()
    base = str(ck / "DisentangledVAE_VCTK_1")
    torch.save(w.model.state_dict(), base + ".pth")
    torch.save({"config": dict(w.adv_config), "adversary": w.adversary.state_dict()}, base + ".adv.pth")
    quiet = lambda *_: None
    plain = make_trainer(B, T)
    assert plain.load_last_model(str(ck), quiet) == 2 and getattr(plain, "adversary", None) is None
    assert plain.load_last_model(str(ck), quiet, restore_adversary=True) == 2
    assert plain.adv_config == w.adv_config and dev_equal(plain.adversary.optimizer.flat_p, w.adversary.optimizer.flat_p)
    other = make_trainer(B, T)
    other.set_speaker_adversary(0.5, n_speakers=SPK, hidden=128)
    with pytest.raises(ValueError, match="speaker adversary"):
        other.load_last_model(str(ck), quiet)


# ------------------------------------------------------------------ the command line
ADV_KEYS = {"Adv/CE", "Adv/Accuracy", "Adv/Weight"}


def _tensors(path):
    sd = torch.load(path, map_location="cpu")
    flat = {}

    def walk(prefix, v):
        if isinstance(v, dict):
            for k, u in v.items():
                walk(f"{prefix}.{k}", u)
        elif isinstance(v, torch.Tensor):
            flat[prefix] = v
    walk("", sd)
    return sd, flat


def test_command_line_resumes_bit_for_bit_and_refuses(tmp_path):
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)   # 16 pairs: 4 steps
    common = ["--train", "true", f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4",
              "--report-interval=1", "--mse_cof=10", "--kl_cof=10", "--seed=3", "--gpu-loader=1"]
    adv = ["--adv-weight", "0.5", "--adv-hidden", "64", "--adv-warmup-steps", "6"]
    one, two = tmp_path / "one", tmp_path / "two"
    child("train", common + ["--epochs=2", f"--log_dir={one}"] + adv)
    child("train", common + ["--epochs=1", f"--log_dir={two}"] + adv)
    child("train", common + ["--epochs=1", f"--log_dir={two}"])          # resumed; without the flags: the saved configuration
    name = "DisentangledVAE_VCTK_2"
    for ext in (".pth", ".adv.pth"):
        sa, fa = _tensors(one / "checkpoints" / (name + ext))
        sb, fb = _tensors(two / "checkpoints" / (name + ext))
        assert set(fa) == set(fb) and fa
        for k in fa:
            assert dev_equal(fa[k], fb[k]), (ext, k)
    assert sa["config"] == sb["config"] == dict(weight=0.5, n_speakers=2, hidden=64, lr=1e-3, warmup_steps=6, seed=3)
    assert sa["adversary"]["optimizer"]["t"] == sb["adversary"]["optimizer"]["t"] == 8
    # the .pth keeps the reference's keys
    plain_keys = set(make_trainer(B, T).model.state_dict())
    assert set(torch.load(one / "checkpoints" / (name + ".pth"), map_location="cpu")) == plain_keys
    ra = [json.loads(line) for line in open(one / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    rb = [json.loads(line) for line in open(two / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert ra == rb and [r["epoch"] for r in ra] == [1, 2]
    for r in ra:
        assert ADV_KEYS <= set(r) and all(math.isfinite(r[k]) for k in ADV_KEYS) and 0.0 <= r["Adv/Accuracy"] <= 1.0
    # four steps an epoch: the last step of epoch e runs after 4 e - 1 others
    assert [r["Adv/Weight"] for r in ra] == [float(np.float32(0.5 * 3 / 6)), 0.5]
    cfg = json.load(open(one / "config.json"))
    assert cfg["adv_weight"] == 0.5 and cfg["adv_hidden"] == 64
    # another classifier on the same run is refused; so is an adversary on a run that has none
    r = child("train", common + ["--epochs=1", f"--log_dir={two}", "--adv-weight", "0.5", "--adv-hidden", "128",
                                 "--adv-warmup-steps", "6"], ok=False)
    assert r.returncode != 0 and "speaker adversary" in r.stderr
    assert not (two / "checkpoints" / "DisentangledVAE_VCTK_3.pth").exists()
    plain = tmp_path / "plain"
    child("train", common + ["--epochs=1", f"--log_dir={plain}"])
    recs = [json.loads(line) for line in open(plain / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert not ADV_KEYS & set(recs[0]) and not (plain / "checkpoints" / "DisentangledVAE_VCTK_1.adv.pth").exists()
    assert not any(k.startswith("adv_") for k in json.load(open(plain / "config.json")))
    r = child("train", common + ["--epochs=1", f"--log_dir={plain}"] + adv, ok=False)
    assert r.returncode != 0 and "adv.pth is missing" in r.stderr
