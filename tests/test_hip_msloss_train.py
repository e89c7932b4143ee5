"""The smoothing penalty on the training step (ConvolutionalMulVAE.set_smoothing_penalty) on the MI355X:
off is the trainer that never heard of it, weights (0, 0) keep the step's bits while the statistics are computed, a warm-up
changes the weights every step under ONE captured graph, the whole-model gradient with the weights on is the feature-off gradient
plus the restatement's dy pushed through the existing backward from the tapped rec_hat, train() reports what the per-step vectors
add up to, the configuration rides in the optimiser's state, the command line writes, resumes and omits what it should, and the
step with every other opt-in feature on beside it, and the bf16 compute mode, replay what they ran eagerly."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import child, dev_equal, make_trainer
import features_ref as F  # noqa: E402
import msloss_ref as R  # noqa: E402

B, T, D = 4, 64, 64
SMOOTH_KEYS = {"Smooth/MS distance dB", "Smooth/GV ratio dB", "Smooth/MS loss", "Smooth/GV loss", "Smooth/Penalty",
               "Smooth/Weight ms", "Smooth/Weight gv"}
BUFS = ("flat_p", "exp_avg", "exp_avg_sq")


@pytest.fixture(scope="module")
def feed():
    from oracle.fill import synthetic_eps, synthetic_pair
    data = [tuple(t.cuda() for t in synthetic_pair(B, T, 700 + i)) for i in range(3)]
    noise = [synthetic_eps(B, seed=800 + i) for i in range(3)]
    return data, noise


def run(w, feed, steps, after=None, ids=None):
    """`steps` training steps on the shared inputs; the losses of each and whatever `after(i)` returns."""
    data, noise = feed
    out, extra = [], []
    for i in range(steps):
        w.model.eps_override = noise[(2 * i) % 3]
        out.append(w.step(*data[i % 3], None if ids is None else ids[i % 3], train=True))
        if after is not None:
            extra.append(after(i))
    return out, extra


@pytest.fixture(scope="module")
def plain(feed):
    """the feature-off trainer after six steps, eager and under a graph: losses and state, computed once"""
    res = {}
    for graph in (False, True):
        w = make_trainer(B, T)
        w.enable_graph(graph)
        losses, _ = run(w, feed, 6)
        res[graph] = (w, losses)
    return res


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_off_is_the_trainer_that_never_called_the_setter(feed, plain, graph):
    a, la = plain[graph]
    b = make_trainer(B, T)
    b.set_smoothing_penalty(2.0, 1.0, warmup_steps=3)
    b.set_smoothing_penalty(None)
    b.enable_graph(graph)
    lb, _ = run(b, feed, 6)
    assert la == lb
    for name in BUFS:
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    x = feed[0][0][0]
    assert a._graph_signature(x) == b._graph_signature(x) and "smooth" not in str(b._graph_signature(x))
    assert b.model.smooth_tap is False and "smoothing_penalty" not in b.optimizer.state_dict()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_zero_weights_keep_the_bits_and_compute_the_statistics(feed, plain, graph):
    a, la = plain[graph]
    b = make_trainer(B, T)
    b.set_smoothing_penalty(0.0)
    b.enable_graph(graph)
    lb, aux = run(b, feed, 6, lambda i: b.smooth_aux.tolist())
    assert la == lb
    for name in BUFS:
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    x = feed[0][0][0]
    assert b._graph_signature(x) == a._graph_signature(x) + (("smooth", D, 0.003),)
    for v in aux:
        assert all(math.isfinite(u) for u in v) and all(u != 0.0 for u in v[:4]) and v[4] == 0.0, v
    assert len({tuple(v) for v in aux}) == 6                                 # every step wrote its own
    assert b._smooth_coef.tolist() == [0.0, 0.0]


def test_warm_up_under_one_graph_equals_eager(feed):
    a, b = make_trainer(B, T), make_trainer(B, T)
    for w in (a, b):
        w.set_smoothing_penalty(300.0, 150.0, warmup_steps=5)
    b.enable_graph(True)
    graphs = []
    la, ca = run(a, feed, 8, lambda i: (a._smooth_coef.tolist(), a.smooth_aux.tolist()))
    lb, cb = run(b, feed, 8, lambda i: (graphs.append(b._graph), (b._smooth_coef.tolist(), b.smooth_aux.tolist()))[1])
    assert la == lb and ca == cb
    for name in BUFS:
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    # one capture (at the second step), replayed to the end although the weights changed before five of the steps
    assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])
    want = [[float(np.float32(v)) for v in a.smooth_weights_at(k)] for k in range(8)]
    assert [c[0] for c in ca] == want
    assert [w[0] for w in want] == [float(np.float32(300.0 * min(1.0, k / 5))) for k in range(8)] and want[5] == [300.0, 150.0]
    assert a.optimizer.t == b.optimizer.t == 8 and a._step_k == 8
    # the penalty the kernel reports is the weights' combination of its own statistics
    for (wm, wg), aux in ca:
        assert math.isclose(aux[4], wm * aux[0] + wg * aux[1], rel_tol=1e-5, abs_tol=1e-6)
        assert math.isclose(aux[2], R.DB * math.sqrt(aux[0]), rel_tol=1e-5)
    # the penalty moves the step: from the second step on (the first ran with weights 0) the run leaves the feature-off one
    c = make_trainer(B, T)
    lc, _ = run(c, feed, 3)
    assert la[0] == lc[0] and la[2] != lc[2]
    # changing the weights alone is no new capture; switching the feature off is
    b.set_smoothing_penalty(1.0, 4.0)
    run(b, feed, 1)
    assert b._graph is graphs[1] and b._smooth_coef.tolist() == [1.0, 4.0]
    b.set_smoothing_penalty(None)
    run(b, feed, 1)
    assert b._graph is not graphs[1]


def _grads(w):
    return {n: w.model.reference_layout(n, p.grad).detach().double().cpu().clone() for n, p in w.model.named_parameters()}


def _is_prebn_conv_bias(name):
    """tests/test_hip_model.py: conv biases in front of a training-mode BatchNorm have a mathematically zero gradient"""
    return name.endswith(".0.conv.bias") or (name.startswith("dec_modules.") and name.endswith(".0.bias"))


def test_whole_model_gradient_is_the_plain_one_plus_the_restatements(feed):
    """One eager step with the weights on, Adam held back: every parameter's gradient against the feature-off gradient plus
    the restatement's float64 dy pushed through the existing backward from the tapped rec_hat.  The tolerances are
    tests/test_hip_model.py's: relative L2 error 5e-3 per parameter, 0.2 absolute where the gradient is mathematically zero.
    The L1 terms are sums over 80 T elements times mse_cof and the penalty is a mean, so the two weights are chosen from the
    REFERENCES (both pushes are linear in them): each term's pushed gradient is 5 % of the feature-off gradient, in the L2
    norm over all parameters.  They are settings, not thresholds."""
    data, noise = feed
    x1, x2 = data[0]
    a = make_trainer(B, T)
    a.model.eps_override = noise[0]
    a.model.smooth_tap = True                       # the alias of rec_hat, with no penalty on it
    seed = torch.zeros(8, device="cuda")
    seed[0] = 1.0
    a.optimizer.zero_grad()
    outs = a.model.forward_full(x1, x2)
    torch.autograd.backward(a.losses_vector_full(x1, x2, *outs), seed)
    g_off = _grads(a)
    X1, X2 = (t.detach().double().cpu().numpy() for t in (x1, x2))

    def pushed(w_ms, w_gv):
        a.optimizer.zero_grad()
        a.model.forward_full(x1, x2)
        (tap,) = a.model.smooth_inputs
        rec_hat = tap.detach().cpu().numpy()
        assert rec_hat.dtype == np.float32 and rec_hat.shape == (2 * B, 80, T)
        r = R.evaluate(rec_hat, X1, X2, D, 0.003, w_ms, w_gv)
        torch.autograd.backward([tap], [torch.tensor(r["dy"], dtype=torch.float32, device="cuda")])
        return r, _grads(a)

    held = [n for n in g_off if not _is_prebn_conv_bias(n)]
    size = lambda g: math.sqrt(sum(float(g[n].norm()) ** 2 for n in held))
    w_ms = float(np.float32(0.05 * size(g_off) / size(pushed(1.0, 0.0)[1])))
    w_gv = float(np.float32(0.05 * size(g_off) / size(pushed(0.0, 1.0)[1])))
    assert math.isfinite(w_ms) and math.isfinite(w_gv) and w_ms > 0 and w_gv > 0
    ref, g_pen = pushed(w_ms, w_gv)
    b = make_trainer(B, T)
    b.set_smoothing_penalty(w_ms, w_gv)
    b.model.eps_override = noise[0]
    b.optimizer.step = lambda **kw: None            # the step without Adam: the gradients stay
    b._eager_train_step(x1, x2)
    assert b._smooth_coef.tolist() == [w_ms, w_gv]
    g_on = _grads(b)
    print(f"weights ({w_ms:.6g}, {w_gv:.6g})")
    bad, moved = [], 0
    for n in g_on:
        want = g_off[n] + g_pen[n]
        err = float((g_on[n] - want).norm())
        ratio = float(g_pen[n].norm()) / max(1e-30, float(g_off[n].norm()))
        print(f"{n}: |g_off| {float(g_off[n].norm()):.4g} |g_pen| / |g_off| {ratio:.3g} err / |want| {err / max(1e-30, float(want.norm())):.3g}")
        if _is_prebn_conv_bias(n):
            if err > 0.2:
                bad.append((n, err))
        elif err > 5e-3 * float(want.norm()):
            bad.append((n, err, float(want.norm())))
        if not _is_prebn_conv_bias(n) and float((g_on[n] - g_off[n]).norm()) > 5e-3 * float(g_off[n].norm()):
            moved += 1
    assert not bad, bad
    assert moved >= 4, "the penalty's gradient must be visible beside the tolerance in four parameters"
    # and the statistics of that step are the restatement's on the step's own rec_hat
    assert np.allclose(b.smooth_aux.cpu().numpy(), ref["stats"], rtol=1e-4, atol=1e-4)


def test_train_reports_what_the_steps_add_up_to(feed):
    data, noise = feed
    w = make_trainer(B, T)
    w.set_smoothing_penalty(200.0, 100.0, warmup_steps=100)
    w.set_kl_schedule("linear", start=1.0, steps=100)           # together with the KL schedule, clipping and the average
    w.optimizer.set_grad_clip(1e4)
    w.optimizer.set_ema(0.99)
    w.enable_graph(True)
    seen, inner = [], w.step_async

    def recording(*a):
        out = inner(*a)
        seen.append(w.smooth_aux.double().cpu().numpy().copy())
        return out
    w.step_async = recording
    loader = [(x1.cpu(), x2.cpu(), torch.zeros(B, dtype=torch.int64)) for x1, x2 in data] * 2          # six steps
    w.train(loader, 1, logging_func=lambda *_: None)
    assert len(seen) == 6 and w.optimizer.t == 6 and w._step_k == 6
    tot = np.sum(seen, axis=0)
    st = w.smooth_stats
    assert set(st) == SMOOTH_KEYS
    for k, name in enumerate(("Smooth/MS loss", "Smooth/GV loss", "Smooth/MS distance dB", "Smooth/GV ratio dB", "Smooth/Penalty")):
        assert st[name] == tot[k] / 6 and math.isfinite(st[name]), name
    assert (st["Smooth/Weight ms"], st["Smooth/Weight gv"]) == w.smooth_weights_at(5) == (10.0, 5.0)
    assert w.kl_stats is not None and w.grad_stats is not None and w.ema_stats is not None


def test_the_configuration_rides_in_the_optimiser_state(feed):
    a = make_trainer(B, T)
    a.set_smoothing_penalty(200.0, 50.0, warmup_steps=6)
    run(a, feed, 2)
    sd = a.optimizer.state_dict()
    assert sd["smoothing_penalty"] == dict(ms_weight=200.0, gv_weight=50.0, window=64, floor=0.003, warmup_steps=6) and sd["t"] == 2
    b = make_trainer(B, T)
    b.set_smoothing_penalty(200.0, 50.0, warmup_steps=6)
    b.optimizer.load_state_dict(sd)                                         # the same configuration: accepted
    b.model.load_state_dict(a.model.state_dict())
    b._step_k = None
    la, _ = run(a, feed, 2)
    lb, _ = run(b, feed, 2)                                                 # ... and continued where the other one is
    assert la == lb
    assert b._smooth_coef.tolist() == a._smooth_coef.tolist() == [float(np.float32(v)) for v in a.smooth_weights_at(3)]
    assert dev_equal(a.optimizer.flat_p, b.optimizer.flat_p)
    for other in (dict(warmup_steps=7), dict(warmup_steps=6, window=32), dict(warmup_steps=6, floor=0.01)):
        c = make_trainer(B, T)
        c.set_smoothing_penalty(200.0, 50.0, **other)
        before = c.optimizer.exp_avg.clone()
        with pytest.raises(ValueError, match="smoothing penalty"):
            c.optimizer.load_state_dict(sd)
        assert dev_equal(c.optimizer.exp_avg, before) and c.optimizer.t == 0
    c.set_smoothing_penalty(None)
    c.optimizer.load_state_dict(sd)                                         # none asked for: nothing to contradict
    assert c.optimizer.t == 2
    for bad in (dict(ms_weight=-1.0), dict(ms_weight=float("nan")), dict(ms_weight=float("inf")),
                dict(ms_weight=1.0, gv_weight=-0.5), dict(ms_weight=1.0, gv_weight=float("inf")),
                dict(ms_weight=1.0, warmup_steps=-1), dict(ms_weight="x"), dict(ms_weight=1.0, window=7),
                dict(ms_weight=1.0, window=6), dict(ms_weight=1.0, window=48), dict(ms_weight=1.0, window=128),
                dict(ms_weight=1.0, floor=0.0), dict(ms_weight=1.0, floor=-1.0), dict(ms_weight=1.0, floor=float("nan"))):
        with pytest.raises(ValueError):
            c.set_smoothing_penalty(**bad)
    assert c.smooth_cfg is None
    c.set_smoothing_penalty(1.0, window=16)
    assert c.smooth_cfg["window"] == 16 and c._graph_signature(feed[0][0][0])[-1] == ("smooth", 16, 0.003)


# ------------------------------------------------------------------ the command line
LOSS_KEYS = {"epoch", "Loss/Reconstruction Loss1", "Loss/Reconstruction Loss2", "Loss/Reconstruction Loss1 hat",
             "Loss/Reconstruction Loss2 hat", "Loss/Z1 KL Loss", "Loss/Z2 KL Loss", "Loss/Z KL Style"}


def test_command_line_writes_resumes_and_refuses(tmp_path):
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)   # 16 pairs: 4 steps
    common = ["--train", "true", f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4",
              "--report-interval=1", "--mse_cof=10", "--kl_cof=10", "--seed=3", "--gpu-loader=1"]
    smo = ["--gv-loss-weight", "100", "--ms-loss-warmup-steps", "12", "--ms-loss-window", "32"]    # alone: --ms-loss-weight 0
    one, two = tmp_path / "one", tmp_path / "two"
    child("train", common + ["--epochs=2", f"--log_dir={one}"] + smo)
    child("train", common + ["--epochs=1", f"--log_dir={two}"] + smo)
    child("train", common + ["--epochs=1", f"--log_dir={two}"])          # resumed; without the flags: the saved configuration
    ra = [json.loads(line) for line in open(one / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    rb = [json.loads(line) for line in open(two / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert ra == rb and [r["epoch"] for r in ra] == [1, 2], "a resumed run continues the uninterrupted one bit for bit"
    for r in ra:
        assert set(r) == LOSS_KEYS | SMOOTH_KEYS, set(r) ^ (LOSS_KEYS | SMOOTH_KEYS)
        assert all(math.isfinite(v) for v in r.values()), r
        assert r["Smooth/Penalty"] != 0.0 and r["Smooth/GV loss"] != 0.0 and r["Smooth/MS distance dB"] > 0.0
    # four steps an epoch: the last step of epoch e runs after 4 e - 1 others
    assert [r["Smooth/Weight gv"] for r in ra] == [100 * (3 / 12), 100 * (7 / 12)] and [r["Smooth/Weight ms"] for r in ra] == [0.0, 0.0]
    name = "DisentangledVAE_VCTK_2"
    sa = torch.load(one / "checkpoints" / (name + ".pth"), map_location="cpu")
    sb = torch.load(two / "checkpoints" / (name + ".pth"), map_location="cpu")
    assert set(sa) == set(make_trainer(B, T).model.state_dict()) and all(dev_equal(sa[k], sb[k]) for k in sa)
    oa = torch.load(one / "checkpoints" / (name + ".opt"), map_location="cpu")
    ob = torch.load(two / "checkpoints" / (name + ".opt"), map_location="cpu")
    saved = dict(ms_weight=0.0, gv_weight=100.0, window=32, floor=0.003, warmup_steps=12)
    assert oa["smoothing_penalty"] == ob["smoothing_penalty"] == saved
    assert oa["t"] == ob["t"] == 8
    cfg = json.load(open(one / "config.json"))
    assert cfg["ms_loss_weight"] is None and cfg["gv_loss_weight"] == 100.0 and cfg["ms_loss_warmup_steps"] == 12
    flags = ("ms_loss_weight", "gv_loss_weight", "ms_loss_window", "ms_loss_floor", "ms_loss_warmup_steps")
    assert not any(k in json.load(open(two / "config.json")) for k in flags)
    # another configuration on the same run is refused where run_training loads the checkpoint; none asked for: the saved one is back
    w = make_trainer(B, T)
    w.set_smoothing_penalty(0.0, 100.0, window=32, warmup_steps=11)
    rng = torch.cuda.get_rng_state()                    # a checkpoint brings its generator state along
    try:
        with pytest.raises(ValueError, match="smoothing penalty"):
            w.load_last_model(str(two / "checkpoints"), logging_func=lambda *_: None)
        w.set_smoothing_penalty(None)
        assert w.load_last_model(str(two / "checkpoints"), logging_func=lambda *_: None) == 3
    finally:
        torch.cuda.set_rng_state(rng)
    assert w.smooth_cfg == saved and w.optimizer.t == 8 and w.model.smooth_tap is True
    # the command line refuses other flags on the same run
    r = child("train", common + ["--epochs=1", f"--log_dir={two}", "--gv-loss-weight", "50"], ok=False)
    assert r.returncode != 0 and "smoothing penalty" in r.stderr
    # --ms-loss-weight 0 alone is the monitor: the statistics beside the losses
    monitor = tmp_path / "monitor"
    child("train", common + ["--epochs=1", f"--log_dir={monitor}", "--ms-loss-weight", "0"])
    rm = json.loads(open(monitor / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl").readline())
    assert set(rm) == LOSS_KEYS | SMOOTH_KEYS and rm["Smooth/Penalty"] == 0.0 and rm["Smooth/MS loss"] != 0.0
    assert rm["Smooth/Weight ms"] == 0.0 and rm["Smooth/Weight gv"] == 0.0
    # flags that make no sense are refused before anything trains
    r = child("train", common + ["--epochs=1", f"--log_dir={tmp_path / 'bad'}", "--ms-loss-weight", "-1"], ok=False)
    assert r.returncode != 0 and "--ms-loss-weight" in r.stderr


# ------------------------------------------------------------------ beside the other features, and in bf16
def _ids():
    gen = torch.Generator().manual_seed(5)
    return [torch.randint(0, 3, (B,), generator=gen) for _ in range(3)]


def test_graph_equals_eager_with_every_feature_on(feed):
    """the KL schedule with free bits, the adversary, the factor penalty, clipping, the weight average AND this penalty: a
    four-root backward under one captured graph, bit for bit what the eager step computes"""
    ids = _ids()
    a, b = make_trainer(B, T), make_trainer(B, T)
    for w in (a, b):
        F.all_on(w, spk=3, max_norm=1e4, free_bits=(0.05, 0.05))
        w.set_smoothing_penalty(300.0, 150.0, warmup_steps=4)
    b.enable_graph(True)
    graphs = []
    la, ca = run(a, feed, 5, lambda i: (a._smooth_coef.tolist(), a.smooth_aux.tolist(), a.factor_aux.tolist()), ids=ids)
    lb, cb = run(b, feed, 5, lambda i: (graphs.append(b._graph), (b._smooth_coef.tolist(), b.smooth_aux.tolist(),
                                                                 b.factor_aux.tolist()))[1], ids=ids)
    assert la == lb and ca == cb
    for name in BUFS:
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
        assert dev_equal(getattr(a.adversary.optimizer, name), getattr(b.adversary.optimizer, name)), "adversary " + name
    assert dev_equal(a.optimizer.ema, b.optimizer.ema) and dev_equal(a.kl_aux, b.kl_aux) and dev_equal(a.adv_out, b.adv_out)
    assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])
    assert [c[0] for c in ca] == [[float(np.float32(v)) for v in a.smooth_weights_at(k)] for k in range(5)]
    assert all(math.isfinite(v) for c in ca for v in c[1] + c[2]) and all(c[1][4] != 0.0 for c in ca[1:])


def test_graph_equals_eager_in_bf16(feed):
    from dvae_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        a, b = make_trainer(B, T), make_trainer(B, T)
        for w in (a, b):
            w.set_smoothing_penalty(300.0, 150.0, warmup_steps=2)
        b.enable_graph(True)
        la, ca = run(a, feed, 4, lambda i: a.smooth_aux.tolist())
        lb, cb = run(b, feed, 4, lambda i: b.smooth_aux.tolist())
        assert la == lb and ca == cb and b._graph is not None
        for name in BUFS:
            assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
        assert all(math.isfinite(v) for c in ca for v in c) and ca[1][4] != 0.0
    finally:
        ops.set_compute_dtype(ops.DEFAULT_COMPUTE_DTYPE)
