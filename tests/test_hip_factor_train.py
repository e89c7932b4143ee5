"""The factor penalty on the training step (ConvolutionalMulVAE.set_factor_penalty) on the MI355X: off
is the trainer that never heard of it, weights (0, 0) keep the step's bits while the statistics are computed, a warm-up changes
the weights every step under ONE captured graph, the whole-model gradient with the weights on is the feature-off gradient plus
the restatement's three gradients pushed through the existing backward, train() reports what the per-step vectors add up to,
the configuration rides in the optimiser's state and the command line writes, resumes and omits what it should."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import child, dev_equal, make_trainer
import factor_ref as R  # noqa: E402

B, T, D, S = 4, 64, 32, 4
FACTOR_KEYS = {"Factor/TC style", "Factor/TC content", "Factor/Shared", "Factor/MI", "Factor/Penalty", "Factor/Weight tc",
               "Factor/Weight shared"}


@pytest.fixture(scope="module")
def feed():
    from oracle.fill import synthetic_eps, synthetic_pair
    data = [tuple(t.cuda() for t in synthetic_pair(B, T, 700 + i)) for i in range(3)]
    noise = [synthetic_eps(B, seed=800 + i) for i in range(3)]
    return data, noise


def run(w, feed, steps, after=None):
    """`steps` training steps on the shared inputs; the losses of each and whatever `after(i)` returns."""
    data, noise = feed
    out, extra = [], []
    for i in range(steps):
        w.model.eps_override = noise[(2 * i) % 3]
        out.append(w.step(*data[i % 3], None, train=True))
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
    b.set_factor_penalty(2.0, 1.0, warmup_steps=3)
    b.set_factor_penalty(None)
    b.enable_graph(graph)
    lb, _ = run(b, feed, 6)
    assert la == lb
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    x = feed[0][0][0]
    assert a._graph_signature(x) == b._graph_signature(x) and "factor" not in str(b._graph_signature(x))
    assert b.model.factor_tap is False and "factor_penalty" not in b.optimizer.state_dict()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_zero_weights_keep_the_bits_and_compute_the_statistics(feed, plain, graph):
    a, la = plain[graph]
    b = make_trainer(B, T)
    b.set_factor_penalty(0.0)
    b.enable_graph(graph)
    lb, aux = run(b, feed, 6, lambda i: b.factor_aux.tolist())
    assert la == lb
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    x = feed[0][0][0]
    assert b._graph_signature(x) == a._graph_signature(x) + (("factor",),)
    for v in aux:
        assert all(math.isfinite(u) for u in v) and all(u != 0.0 for u in v[:4]) and v[4] == 0.0, v
    assert len({tuple(v) for v in aux}) == 6                                 # every step wrote its own
    assert b._fac_coef.tolist() == [0.0, 0.0]


def test_warm_up_under_one_graph_equals_eager(feed):
    a, b = make_trainer(B, T), make_trainer(B, T)
    for w in (a, b):
        w.set_factor_penalty(3.0, 1.5, warmup_steps=5)
    b.enable_graph(True)
    graphs = []
    la, ca = run(a, feed, 8, lambda i: (a._fac_coef.tolist(), a.factor_aux.tolist()))
    lb, cb = run(b, feed, 8, lambda i: (graphs.append(b._graph), (b._fac_coef.tolist(), b.factor_aux.tolist()))[1])
    assert la == lb and ca == cb
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    # one capture (at the second step), replayed to the end although the weights changed before five of the steps
    assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])
    want = [[float(np.float32(v)) for v in a.factor_weights_at(k)] for k in range(8)]
    assert [c[0] for c in ca] == want
    assert [w[0] for w in want] == [float(np.float32(3.0 * min(1.0, k / 5))) for k in range(8)] and want[5] == [3.0, 1.5]
    assert a.optimizer.t == b.optimizer.t == 8 and a._step_k == 8
    # the penalty the kernel reports is the weights' combination of its own statistics
    for (wt, ws), aux in ca:
        assert math.isclose(aux[4], wt * (aux[0] + aux[1]) + ws * aux[2], rel_tol=1e-5, abs_tol=1e-6)
    # the penalty moves the step: from the second step on (the first ran with weights 0) the run leaves the feature-off one
    c = make_trainer(B, T)
    lc, _ = run(c, feed, 3)
    assert la[0] == lc[0] and la[2] != lc[2]
    # changing the weights alone is no new capture; switching the feature off is
    b.set_factor_penalty(1.0, 4.0)
    run(b, feed, 1)
    assert b._graph is graphs[1] and b._fac_coef.tolist() == [1.0, 4.0]
    b.set_factor_penalty(None)
    run(b, feed, 1)
    assert b._graph is not graphs[1]


def _grads(w):
    return {n: w.model.reference_layout(n, p.grad).detach().double().cpu().clone() for n, p in w.model.named_parameters()}


def _is_prebn_conv_bias(name):
    """tests/test_hip_model.py: conv biases in front of a training-mode BatchNorm have a mathematically zero gradient"""
    return name.endswith(".0.conv.bias") or (name.startswith("dec_modules.") and name.endswith(".0.bias"))


def test_whole_model_gradient_is_the_plain_one_plus_the_restatements(feed):
    """One eager step with the weights on, Adam held back: every parameter's gradient against the feature-off gradient plus
    the restatement's float64 dz, dq_mu, dq_lv pushed through dvae_latent_bwd and the encoder by autograd on the existing ops.
    The tolerances are tests/test_hip_model.py's: relative L2 error 5e-3 per parameter, 0.2 absolute where the gradient is
    mathematically zero."""
    data, noise = feed
    x1, x2 = data[0]
    w_tc, w_sh = 40.0, 25.0
    a = make_trainer(B, T)
    a.model.eps_override = noise[0]
    a.model.factor_tap = True                       # the aliases of (z, q_mu, q_lv), with no penalty on them
    seed = torch.zeros(8, device="cuda")
    seed[0] = 1.0
    a.optimizer.zero_grad()
    outs = a.model.forward_full(x1, x2)
    torch.autograd.backward(a.losses_vector_full(x1, x2, *outs), seed)
    g_off = _grads(a)
    a.optimizer.zero_grad()
    a.model.forward_full(x1, x2)
    z, mu, lv = a.model.factor_inputs
    ref = R.gradients(*(t.detach().double().cpu().numpy() for t in (z, mu, lv)), S, w_tc, w_sh)
    torch.autograd.backward([z, mu, lv], [torch.tensor(g_, dtype=torch.float32, device="cuda") for g_ in ref])
    g_pen = _grads(a)
    encoder = lambda n: n.startswith(("enc_", "style.", "content."))       # the penalty reaches nothing behind z
    b = make_trainer(B, T)
    b.set_factor_penalty(w_tc, w_sh)
    b.model.eps_override = noise[0]
    b.optimizer.step = lambda **kw: None            # the step without Adam: the gradients stay
    b._eager_train_step(x1, x2)
    assert b._fac_coef.tolist() == [w_tc, w_sh]
    g_on = _grads(b)
    bad, moved = [], 0
    for n in g_on:
        want = g_off[n] + (g_pen[n] if encoder(n) else 0.0)
        err = float((g_on[n] - want).norm())
        ratio = float(g_pen[n].norm()) / max(1e-30, float(g_off[n].norm())) if encoder(n) else 0.0
        print(f"{n}: |g_off| {float(g_off[n].norm()):.4g} |g_pen| / |g_off| {ratio:.3g} err / |want| {err / max(1e-30, float(want.norm())):.3g}")
        if _is_prebn_conv_bias(n):
            if err > 0.2:
                bad.append((n, err))
        elif err > 5e-3 * float(want.norm()):
            bad.append((n, err, float(want.norm())))
        if encoder(n) and not _is_prebn_conv_bias(n) and float((g_on[n] - g_off[n]).norm()) > 5e-3 * float(g_off[n].norm()):
            moved += 1
    assert not bad, bad
    assert moved >= 4, "the penalty's gradient must be visible beside the tolerance in the encoder's parameters"
    # and the statistics of that step are the restatement's on the step's own latents
    f = R.forward(*(t.detach().double().cpu().numpy() for t in (z, mu, lv)), S, w_tc, w_sh)
    assert np.allclose(b.factor_aux.cpu().numpy(), f["stats"], rtol=1e-4, atol=1e-4)


def test_train_reports_what_the_steps_add_up_to(feed):
    data, noise = feed
    w = make_trainer(B, T)
    w.set_factor_penalty(2.0, 1.0, warmup_steps=100)
    w.set_kl_schedule("linear", start=1.0, steps=100)           # together with the KL schedule, clipping and the average
    w.optimizer.set_grad_clip(1e4)
    w.optimizer.set_ema(0.99)
    w.enable_graph(True)
    seen, inner = [], w.step_async

    def recording(*a):
        out = inner(*a)
        seen.append(w.factor_aux.double().cpu().numpy().copy())
        return out
    w.step_async = recording
    loader = [(x1.cpu(), x2.cpu(), torch.zeros(B, dtype=torch.int64)) for x1, x2 in data] * 2          # six steps
    w.train(loader, 1, logging_func=lambda *_: None)
    assert len(seen) == 6 and w.optimizer.t == 6 and w._step_k == 6
    tot = np.sum(seen, axis=0)
    st = w.factor_stats
    assert set(st) == FACTOR_KEYS
    for k, name in enumerate(("Factor/TC style", "Factor/TC content", "Factor/Shared", "Factor/MI", "Factor/Penalty")):
        assert st[name] == tot[k] / 6 and math.isfinite(st[name]), name
    assert (st["Factor/Weight tc"], st["Factor/Weight shared"]) == w.factor_weights_at(5) == (0.1, 0.05)
    assert w.kl_stats is not None and w.grad_stats is not None and w.ema_stats is not None


def test_the_configuration_rides_in_the_optimiser_state(feed):
    a = make_trainer(B, T)
    a.set_factor_penalty(2.0, 0.5, warmup_steps=6)
    run(a, feed, 2)
    sd = a.optimizer.state_dict()
    assert sd["factor_penalty"] == dict(tc_weight=2.0, shared_weight=0.5, warmup_steps=6) and sd["t"] == 2
    b = make_trainer(B, T)
    b.set_factor_penalty(2.0, 0.5, warmup_steps=6)
    b.optimizer.load_state_dict(sd)                                         # the same configuration: accepted
    b.model.load_state_dict(a.model.state_dict())
    b._step_k = None
    la, _ = run(a, feed, 2)
    lb, _ = run(b, feed, 2)                                                 # ... and continued where the other one is
    assert la == lb and b._fac_coef.tolist() == a._fac_coef.tolist() == [float(np.float32(v)) for v in a.factor_weights_at(3)]
    assert dev_equal(a.optimizer.flat_p, b.optimizer.flat_p)
    c = make_trainer(B, T)
    c.set_factor_penalty(2.0, 0.5, warmup_steps=7)
    before = c.optimizer.exp_avg.clone()
    with pytest.raises(ValueError, match="factor penalty"):
        c.optimizer.load_state_dict(sd)
    assert dev_equal(c.optimizer.exp_avg, before) and c.optimizer.t == 0
    c.set_factor_penalty(None)
    c.optimizer.load_state_dict(sd)                                         # none asked for: nothing to contradict
    assert c.optimizer.t == 2
    for bad in (dict(tc_weight=-1.0), dict(tc_weight=float("nan")), dict(tc_weight=float("inf")),
                dict(tc_weight=1.0, shared_weight=-0.5), dict(tc_weight=1.0, shared_weight=float("inf")),
                dict(tc_weight=1.0, warmup_steps=-1), dict(tc_weight="x")):
        with pytest.raises(ValueError):
            c.set_factor_penalty(**bad)
    wide = make_trainer(B, T)
    wide.model.latent_dim = 68
    with pytest.raises(ValueError, match="latent dimensions"):
        wide.set_factor_penalty(1.0)


# ------------------------------------------------------------------ the command line
LOSS_KEYS = {"epoch", "Loss/Reconstruction Loss1", "Loss/Reconstruction Loss2", "Loss/Reconstruction Loss1 hat",
             "Loss/Reconstruction Loss2 hat", "Loss/Z1 KL Loss", "Loss/Z2 KL Loss", "Loss/Z KL Style"}


def test_command_line_writes_resumes_and_refuses(tmp_path):
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)   # 16 pairs: 4 steps
    common = ["--train", "true", f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4",
              "--report-interval=1", "--mse_cof=10", "--kl_cof=10", "--seed=3", "--gpu-loader=1"]
    fac = ["--shared-weight", "1", "--factor-warmup-steps", "12"]        # --shared-weight alone: it implies --tc-weight 0
    one, two = tmp_path / "one", tmp_path / "two"
    child("train", common + ["--epochs=2", f"--log_dir={one}"] + fac)
    child("train", common + ["--epochs=1", f"--log_dir={two}"] + fac)
    child("train", common + ["--epochs=1", f"--log_dir={two}"])          # resumed; without the flags: the saved configuration
    ra = [json.loads(line) for line in open(one / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    rb = [json.loads(line) for line in open(two / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert ra == rb and [r["epoch"] for r in ra] == [1, 2], "a resumed run continues the uninterrupted one bit for bit"
    for r in ra:
        assert set(r) == LOSS_KEYS | FACTOR_KEYS, set(r) ^ (LOSS_KEYS | FACTOR_KEYS)
        assert all(math.isfinite(v) for v in r.values()), r
        assert r["Factor/Penalty"] != 0.0 and r["Factor/Shared"] != 0.0
    # four steps an epoch: the last step of epoch e runs after 4 e - 1 others
    assert [r["Factor/Weight shared"] for r in ra] == [3 / 12, 7 / 12] and [r["Factor/Weight tc"] for r in ra] == [0.0, 0.0]
    name = "DisentangledVAE_VCTK_2"
    sa = torch.load(one / "checkpoints" / (name + ".pth"), map_location="cpu")
    sb = torch.load(two / "checkpoints" / (name + ".pth"), map_location="cpu")
    assert set(sa) == set(make_trainer(B, T).model.state_dict()) and all(dev_equal(sa[k], sb[k]) for k in sa)
    oa = torch.load(one / "checkpoints" / (name + ".opt"), map_location="cpu")
    ob = torch.load(two / "checkpoints" / (name + ".opt"), map_location="cpu")
    assert oa["factor_penalty"] == ob["factor_penalty"] == dict(tc_weight=0.0, shared_weight=1.0, warmup_steps=12)
    assert oa["t"] == ob["t"] == 8
    cfg = json.load(open(one / "config.json"))
    assert cfg["tc_weight"] is None and cfg["shared_weight"] == 1.0 and cfg["factor_warmup_steps"] == 12
    assert not any(k in json.load(open(two / "config.json")) for k in ("tc_weight", "shared_weight", "factor_warmup_steps"))
    # another configuration on the same run is refused where run_training loads the checkpoint; none asked for: the saved one is back
    w = make_trainer(B, T)
    w.set_factor_penalty(0.0, 1.0, warmup_steps=11)
    rng = torch.cuda.get_rng_state()                    # a checkpoint brings its generator state along
    try:
        with pytest.raises(ValueError, match="factor penalty"):
            w.load_last_model(str(two / "checkpoints"), logging_func=lambda *_: None)
        w.set_factor_penalty(None)
        assert w.load_last_model(str(two / "checkpoints"), logging_func=lambda *_: None) == 3
    finally:
        torch.cuda.set_rng_state(rng)
    assert w.factor_cfg == dict(tc_weight=0.0, shared_weight=1.0, warmup_steps=12) and w.optimizer.t == 8
    assert w.model.factor_tap is True
    # --tc-weight 0 alone is the monitor: the statistics beside the losses
    monitor = tmp_path / "monitor"
    child("train", common + ["--epochs=1", f"--log_dir={monitor}", "--tc-weight", "0"])
    rm = json.loads(open(monitor / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl").readline())
    assert set(rm) == LOSS_KEYS | FACTOR_KEYS and rm["Factor/Penalty"] == 0.0 and rm["Factor/Shared"] != 0.0
    assert rm["Factor/Weight tc"] == 0.0 and rm["Factor/Weight shared"] == 0.0
    # flags that make no sense are refused before anything trains
    r = child("train", common + ["--epochs=1", f"--log_dir={tmp_path / 'bad'}", "--tc-weight", "-1"], ok=False)
    assert r.returncode != 0 and "--tc-weight" in r.stderr
