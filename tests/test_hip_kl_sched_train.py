"""The KL schedule and free bits on the training step (ConvolutionalMulVAE.set_kl_schedule) on the MI355X: "constant" is the
step without the feature bit for bit, a ramp changes the weight every step under ONE captured graph, free bits above every
dimension's KL train like kl_cof = 0, train() reports what the per-step vectors add up to, the schedule rides in the
optimiser's state and the command line writes, resumes and omits what it should."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import child, dev_equal, make_trainer

B, T, D = 4, 64, 32


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


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_constant_is_the_step_without_the_feature(feed, graph):
    a, b = make_trainer(B, T), make_trainer(B, T)
    b.set_kl_schedule("constant")
    for w in (a, b):
        w.enable_graph(graph)
    la, _ = run(a, feed, 6)
    lb, _ = run(b, feed, 6)
    assert la == lb
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    assert ("kl_sched", False) in b._graph_signature(feed[0][0][0]) and 10.0 not in b._graph_signature(feed[0][0][0])
    assert a._graph_signature(feed[0][0][0])[3:5] == (10.0, 10.0) and "kl_sched" not in str(a._graph_signature(feed[0][0][0]))
    aux = b.kl_aux.tolist()
    assert aux[2:4] == [0.0, 0.0] and aux[4 + 2 * D:] == [1.0] * (2 * D) and aux[0:2] == list(lb[-1][5:7])
    assert math.isclose(sum(aux[4:4 + D]), lb[-1][5], rel_tol=1e-5)


def test_linear_ramp_under_one_graph_equals_eager(feed):
    a, b = make_trainer(B, T), make_trainer(B, T)
    for w in (a, b):
        w.set_kl_schedule("linear", start=0.0, steps=5)
    b.enable_graph(True)
    graphs = []
    la, ca = run(a, feed, 8, lambda i: a._kl_coef[:2].tolist())
    lb, cb = run(b, feed, 8, lambda i: (graphs.append(b._graph), b._kl_coef[:2].tolist())[1])
    assert la == lb
    for name in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), name
    # one capture (at the second step), replayed to the end although the weight changed before six of the steps
    assert graphs[0] is None and graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])
    want = [[10.0, float(np.float32(a.kl_weight_at(k)))] for k in range(8)]
    assert ca == want and cb == want and [w[1] for w in want[:6]] == [0.0, 2.0, 4.0, 6.0, 8.0, 10.0]
    assert a.optimizer.t == b.optimizer.t == 8 and a._step_k == 8
    # the first step's weight is 0: LOSS is mse_cof times the four L1 terms of its own vector, exactly
    l0 = [np.float32(v) for v in la[0]]
    assert np.float32(la[0][0]) == np.float32(10.0) * (((l0[1] + l0[2]) + l0[3]) + l0[4])
    assert la[0][5] > 0 and la[0][6] > 0                        # the raw terms are reported all the same
    # switching free bits on changes the launches' arguments: captured again
    b.set_kl_schedule("linear", start=0.0, steps=5, free_bits=0.01)
    run(b, feed, 1)
    assert b._graph is not None and b._graph is not graphs[1]


def test_free_bits_above_every_kl_train_like_kl_cof_zero(feed):
    a, b = make_trainer(B, T), make_trainer(B, T)
    a.kl_cof = 0.0
    b.set_kl_schedule("constant", free_bits=1e6)
    la, _ = run(a, feed, 3)
    lb, counts = run(b, feed, 3, lambda i: b.kl_aux[2:4].tolist())
    assert counts == [[float(D), float(D)]] * 3
    assert torch.equal(a.optimizer.flat_p, b.optimizer.flat_p)           # as numbers
    assert [v[1:] for v in la] == [v[1:] for v in lb]                     # the raw terms; LOSS carries the lambdas
    assert all(math.isclose(v[0] - u[0], 10.0 * 2 * D * 1e6, rel_tol=1e-5) for u, v in zip(la, lb))


def test_train_reports_what_the_steps_add_up_to(feed):
    data, noise = feed
    w = make_trainer(B, T)
    w.set_kl_schedule("constant")
    w.model.eps_override = noise[0]
    w.step(*data[0], None, train=True)
    lam = float(np.median(w.kl_aux[4:4 + D].cpu().numpy()))
    assert lam > 0
    w.set_kl_schedule("linear", start=1.0, steps=100, free_bits=lam)
    w.enable_graph(True)
    seen, inner = [], w.step_async

    def recording(*a):
        out = inner(*a)
        seen.append(w.kl_aux.double().cpu().numpy().copy())
        return out
    w.step_async = recording
    loader = [(x1.cpu(), x2.cpu(), torch.zeros(B, dtype=torch.int64)) for x1, x2 in data] * 2          # six steps
    lines = []
    w.train(loader, 1, logging_func=lines.append)
    assert len(seen) == 6 and w.optimizer.t == 7 and w._step_k == 7
    tot = np.zeros(2 + 2 * D)
    for a in seen:
        tot += a[2:4 + 2 * D]
    assert 0 < tot[0] < 6 * D and 0 < tot[1] < 6 * D                         # a moderate lambda: some free, some not
    st, dims = w.kl_stats, w.kl_dims
    assert st["KL/Free dims z1"] == tot[0] / 6 and st["KL/Free dims z2"] == tot[1] / 6
    assert dims["z1"] == list(tot[2:2 + D] / 6) and dims["z2"] == list(tot[2 + D:] / 6) and dims["steps"] == 6
    assert st["KL/Active dims"] == int((tot[2:2 + D] / 6 > 0.01).sum())
    assert st["KL/Weight"] == w.kl_weight_at(6) and 1.5 < st["KL/Weight"] < 1.6      # the epoch's last step ran after six others


def test_the_schedule_rides_in_the_optimiser_state(feed):
    a = make_trainer(B, T)
    a.set_kl_schedule("cyclical", start=0.5, steps=12, cycles=3, ratio=0.5, free_bits=(0.0, 0.05))
    run(a, feed, 2)
    sd = a.optimizer.state_dict()
    assert sd["kl_schedule"] == dict(kind="cyclical", start=0.5, steps=12, cycles=3, ratio=0.5, free_bits=[0.0] * 4 + [0.05] * 28)
    assert sd["t"] == 2
    b = make_trainer(B, T)
    assert "kl_schedule" not in b.optimizer.state_dict()
    b.set_kl_schedule("cyclical", start=0.5, steps=12, cycles=3, ratio=0.5, free_bits=(0.0, 0.05))
    b.optimizer.load_state_dict(sd)                                         # the same schedule: accepted
    assert b.optimizer.t == 2
    b.model.load_state_dict(a.model.state_dict())
    b._step_k = None
    la, _ = run(a, feed, 2)
    data, noise = feed
    lb = []
    for i in range(2):                                                      # ... and continued where the other one is
        b.model.eps_override = noise[(2 * i) % 3]
        lb.append(b.step(*data[i % 3], None, train=True))
    assert la == lb and b._kl_coef[:2].tolist() == a._kl_coef[:2].tolist() == [10.0, float(np.float32(a.kl_weight_at(3)))]
    c = make_trainer(B, T)
    c.set_kl_schedule("cyclical", start=0.5, steps=12, cycles=4, ratio=0.5, free_bits=(0.0, 0.05))
    before = c.optimizer.exp_avg.clone()
    with pytest.raises(ValueError, match="KL schedule"):
        c.optimizer.load_state_dict(sd)
    assert dev_equal(c.optimizer.exp_avg, before) and c.optimizer.t == 0
    c.set_kl_schedule(None)
    c.optimizer.load_state_dict(sd)                                         # none asked for: nothing to contradict
    assert c.optimizer.t == 2
    with pytest.raises(ValueError):
        c.set_kl_schedule(None, free_bits=0.1)
    with pytest.raises(ValueError):
        c.set_kl_schedule("linear", steps=0)


# ------------------------------------------------------------------ the command line
LOSS_KEYS = {"epoch", "Loss/Reconstruction Loss1", "Loss/Reconstruction Loss2", "Loss/Reconstruction Loss1 hat",
             "Loss/Reconstruction Loss2 hat", "Loss/Z1 KL Loss", "Loss/Z2 KL Loss", "Loss/Z KL Style"}
KL_KEYS = {"KL/Weight", "KL/Free dims z1", "KL/Free dims z2", "KL/Active dims"}


def test_command_line_writes_resumes_and_omits(tmp_path):
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)   # 16 pairs: 4 steps
    common = ["--train", "true", f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4",
              "--report-interval=2", "--mse_cof=10", "--kl_cof=10", "--seed=3"]
    kl = ["--kl-schedule", "cyclical", "--kl-warmup-steps", "12", "--kl-cycles", "2", "--free-bits-content", "0.05"]
    log = tmp_path / "kl"
    scalars = log / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl"
    child("train", common + ["--epochs=2", f"--log_dir={log}"] + kl)
    recs = [json.loads(line) for line in open(scalars)]
    assert [r["epoch"] for r in recs] == [1, 2]
    for r in recs:
        assert set(r) == LOSS_KEYS | KL_KEYS, set(r) ^ (LOSS_KEYS | KL_KEYS)
        assert all(math.isfinite(v) for v in r.values()), r
        assert 0 <= r["KL/Free dims z1"] <= D and 0 <= r["KL/Active dims"] <= D
    from dvae_amd.kl_schedule import KLSchedule
    s = KLSchedule("cyclical", 0.0, 12, 2, 0.5)
    # four steps an epoch: the last step of epoch e runs after 4 e - 1 others
    assert [r["KL/Weight"] for r in recs] == [s.weight_at(3, 1, 10.0), s.weight_at(7, 2, 10.0)]
    dims = json.load(open(log / "kl_dims.json"))
    assert dims["epoch"] == 2 and len(dims["z1"]) == len(dims["z2"]) == D and all(v >= 0 for v in dims["z1"] + dims["z2"])
    cfg = json.load(open(log / "config.json"))
    assert cfg["kl_schedule"] == "cyclical" and cfg["free_bits_content"] == 0.05 and cfg["kl_warmup_steps"] == 12
    # a second invocation resumes at epoch 3 and continues the schedule; without the flags the saved one is restored
    child("train", common + ["--epochs=1", f"--log_dir={log}"])
    recs = [json.loads(line) for line in open(scalars)]
    assert [r["epoch"] for r in recs] == [1, 2, 3] and set(recs[2]) == LOSS_KEYS | KL_KEYS
    assert recs[2]["KL/Weight"] == s.weight_at(11, 3, 10.0)
    # another schedule on the same run is refused where run_training loads the checkpoint; none asked for: the saved one is back
    w = make_trainer(B, T)
    w.set_kl_schedule("linear", steps=12)
    rng = torch.cuda.get_rng_state()                    # a checkpoint brings its generator state along
    try:
        with pytest.raises(ValueError, match="KL schedule"):
            w.load_last_model(str(log / "checkpoints"), logging_func=lambda *_: None)
        w.set_kl_schedule(None)
        assert w.load_last_model(str(log / "checkpoints"), logging_func=lambda *_: None) == 3
    finally:
        torch.cuda.set_rng_state(rng)
    assert w.kl_sched.params() == dict(s.params(), free_bits=[0.0] * 4 + [0.05] * 28) and w.optimizer.t == 8
    # without the flags: none of the keys, no file
    plain = tmp_path / "plain"
    child("train", common + ["--epochs=1", "--do-not-resume", f"--log_dir={plain}"])
    recs = [json.loads(line) for line in open(plain / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    assert set(recs[0]) == LOSS_KEYS and not (plain / "kl_dims.json").exists()
    assert not any(k.startswith("kl_") or k.startswith("free_bits") for k in json.load(open(plain / "config.json")) if k != "kl_cof")
