"""The opt-in features of the train step (dvae_amd.step_features) on the host: the warm-up ramp, the host logic of a step
(one count, one send, only what changed), the epoch records and the optimiser's sidecar.  The setters refuse a CPU device, so
the GPU suites hold these properties end to end; the table makes them testable here, on stand-in features whose buffers are
CPU tensors."""
import math

import pytest
import torch


def tiny_trainer():
    import dvae_amd  # noqa: F401
    from dvae_amd.model.variational_base_vae import VariationalBaseModelVAE

    class Opt:
        """counts the reads of `t` (on the device: a device-to-host sync)"""
        betas, eps = (0.9, 0.999), 1e-8

        def __init__(self):
            self.steps, self.reads = 5, 0

        @property
        def t(self):
            self.reads += 1
            return self.steps

    class Sender:
        def __init__(self):
            self.sent = []

        def send(self, items):
            self.sent.append([(dst.data_ptr(), dst.numel(), tuple(vals)) for dst, vals in items])

    class Tiny(VariationalBaseModelVAE):
        def __init__(self):
            super().__init__("VCTK", 64, 80, 1, 32, 1e-4, torch.device("cpu"), 500, 4)
            self.model = torch.nn.Linear(4, 4)
            self.mse_cof, self.kl_cof = 10, 8.0
            self.optimizer, self._sender = Opt(), Sender()

    return Tiny()


RAMPED = (("adv", ("weight",)), ("factor", ("tc_weight", "shared_weight")), ("smooth", ("ms_weight", "gv_weight")))


@pytest.mark.parametrize("name,keys", RAMPED)
@pytest.mark.parametrize("n", [0, 1, 7])
def test_the_ramp_is_the_literal_expression(name, keys, n):
    t = tiny_trainer()
    f = t.features[name]
    f.cfg = dict(zip(keys, (0.7, 0.3)), warmup_steps=n, window=16, floor=0.003)
    at = {"adv": lambda k: (t.adv_weight_at(k),), "factor": t.factor_weights_at, "smooth": t.smooth_weights_at}[name]
    for k in sorted({max(0, k) for k in (0, 1, n - 1, n, n + 1, 10 * n)}):
        want = tuple(w if n <= 0 else w * min(1.0, k / n) for w in (0.7, 0.3)[:len(keys)])
        assert f.weights_at(k) == f.weights_at(k, 3) == at(k) == want, (k, f.weights_at(k), want)


def test_the_kl_feature_delegates_to_the_schedule_and_prepends_mse_cof():
    from dvae_amd.kl_schedule import KLSchedule
    t = tiny_trainer()
    f = t.features["kl"]
    for kind, kw in (("constant", {}), ("linear", dict(start=1.0, steps=6)), ("cyclical", dict(start=0.5, steps=12, cycles=3)),
                     ("double", dict(start=0.25))):
        f.sched = KLSchedule(kind, **kw)
        f.cfg = f.sched.params()
        for k in (0, 1, 5, 6, 7, 60):
            for epoch in (1, 4):
                assert f.weights_at(k, epoch) == (float(t.mse_cof), KLSchedule(kind, **kw).weight_at(k, epoch, t.kl_cof))
    assert f.signature() == (("kl_sched", False),) and f.device_cofs and not f.rooted


def stand_ins(t):
    """two features of the table's kind whose device scalars are CPU tensors and whose weights the test sets"""
    from dvae_amd.step_features import StepFeature

    class StandIn(StepFeature):
        rooted = False

        def __init__(self, trainer, name, rank, n):
            super().__init__(trainer)
            self.name, self.rank, self.coef, self.value = name, rank, torch.zeros(n), (0.0,) * n

        def signature(self):
            return ((self.name, len(self.value)),)

        def weights_at(self, k, epoch=1):
            return self.value

    t.features = {"a": StandIn(t, "a", 1, 2), "b": StandIn(t, "b", 0, 1)}
    return t.features["a"], t.features["b"]


def test_the_steps_host_logic():
    t = tiny_trainer()
    a, b = stand_ins(t)
    opt, sent = t.optimizer, t._sender.sent
    x = torch.zeros(2, 80, 64)
    plain = t._graph_signature(x)
    # nothing on: no read of t, no count, nothing sent, nothing added to the signature
    t._sync_step_coefs()
    assert opt.reads == 0 and t._step_k is None and sent == [] and not t._features_on()
    a.cfg, b.cfg = {}, {}
    assert t._graph_signature(x) == plain + b.signature() + a.signature() == plain + (("b", 1), ("a", 2))
    b.cfg = None
    assert t._graph_signature(x) == plain + (("a", 2),)
    b.cfg = {}
    # on: one read of t over several steps, the count advances by one per call, one send carrying both (in rank order)
    a.value, b.value = (1.0, 2.0), (3.0,)
    t._sync_step_coefs()
    assert opt.reads == 1 and t._step_k == 6
    assert sent == [[(b.coef.data_ptr(), 1, (3.0,)), (a.coef.data_ptr(), 2, (1.0, 2.0))]]
    # the same weights again: nothing is sent
    t._sync_step_coefs()
    assert opt.reads == 1 and t._step_k == 7 and len(sent) == 1
    # one feature's weights changed: that feature only
    a.value = (1.0, 2.5)
    t._sync_step_coefs()
    assert opt.reads == 1 and t._step_k == 8 and sent[1:] == [[(a.coef.data_ptr(), 2, (1.0, 2.5))]]
    assert a.weights == a.sent == (1.0, 2.5) and b.weights == b.sent == (3.0,)
    # a setter: t is read again, and that feature is sent even though its value is what it was
    opt.steps = 40
    t._feature_set("b")
    assert t._step_k is None and b.sent is None and b.weights is None and a.sent == (1.0, 2.5)
    t._sync_step_coefs()
    assert opt.reads == 2 and t._step_k == 41 and sent[2:] == [[(b.coef.data_ptr(), 1, (3.0,))]]
    # everything off again: the plain trainer
    a.cfg = b.cfg = None
    t._sync_step_coefs()
    assert opt.reads == 2 and t._step_k == 41 and len(sent) == 3 and t._graph_signature(x) == plain


def test_the_epoch_records():
    t = tiny_trainer()
    adv = t.features["adv"].stats([6.0, 4.0, 3.0, 0.0], 3, (0.25,))
    assert adv == {"Adv/CE": 6.0 / 4.0, "Adv/Accuracy": 3.0 / 4.0, "Adv/Weight": 0.25}
    none = t.features["adv"].stats([0.0, 0.0, 0.0, 0.0], 3, (0.25,))
    assert set(none) == set(adv) and math.isnan(none["Adv/CE"]) and math.isnan(none["Adv/Accuracy"]) and none["Adv/Weight"] == 0.25
    f, n = [1.0, 2.0, 3.0, 4.0, 5.0], 3
    assert t.features["factor"].stats(f, n, (0.7, 0.3)) == {
        "Factor/TC style": f[0] / n, "Factor/TC content": f[1] / n, "Factor/Shared": f[2] / n, "Factor/MI": f[3] / n,
        "Factor/Penalty": f[4] / n, "Factor/Weight tc": 0.7, "Factor/Weight shared": 0.3}
    assert t.features["smooth"].stats(f, n, (0.7, 0.3)) == {
        "Smooth/MS distance dB": f[2] / n, "Smooth/GV ratio dB": f[3] / n, "Smooth/MS loss": f[0] / n,
        "Smooth/GV loss": f[1] / n, "Smooth/Penalty": f[4] / n, "Smooth/Weight ms": 0.7, "Smooth/Weight gv": 0.3}
    # no step at all divides by one
    assert t.features["factor"].stats(f, 0, (0.7, 0.3))["Factor/Penalty"] == 5.0
    # KL: two free counts, then the per-dimension KL of z1 [D] and of z2 [D]; D = 3
    kl = t.features["kl"]
    k = [4.0, 2.0, 0.9, 0.02, 0.06, 8.0, 8.0, 0.0]
    assert kl.stats(k, 2, (10.0, 1.5), epoch=7) == {"KL/Weight": 1.5, "KL/Free dims z1": 2.0, "KL/Free dims z2": 1.0,
                                                     "KL/Active dims": 2}         # 0.45 and 0.03 of z1; 0.01 is not above 0.01
    assert kl.dims == {"epoch": 7, "steps": 2, "z1": [0.45, 0.01, 0.03], "z2": [4.0, 4.0, 0.0]}
    kl.report = kl.dims = None
    assert kl.dims is None and kl.report is None and t.kl_dims is None and t.kl_stats is None


KL_CFG = {"kind": "linear", "start": 1.0, "steps": 6, "cycles": 4, "ratio": 0.5, "free_bits": [0.5, 0.5, 0.25]}
FACTOR_CFG = {"tc_weight": 3.0, "shared_weight": 1.5, "warmup_steps": 7}
SMOOTH_CFG = {"ms_weight": 1.0, "gv_weight": 4.0, "window": 16, "floor": 0.003, "warmup_steps": 5}
SIDECAR = (("kl_schedule", KL_CFG, "KL schedule"), ("factor_penalty", FACTOR_CFG, "factor penalty"),
           ("smoothing_penalty", SMOOTH_CFG, "smoothing penalty"))


def test_the_configurations_ride_in_the_optimiser_state():
    import dvae_amd  # noqa: F401
    from dvae_amd.optim import FlatAdam
    make = lambda: FlatAdam([("lin.weight", torch.nn.Parameter(torch.zeros(4, 6)))], lr=1e-3)
    a = make()
    assert not any(key in a.state_dict() for key, _, _ in SIDECAR)
    for key, cfg, _ in SIDECAR:
        a.step_features[key] = dict(cfg)
    sd = a.state_dict()
    for key, cfg, _ in SIDECAR:
        assert sd[key] == cfg and sd[key] is not a.step_features[key]
    make().load_state_dict(sd)                          # a run that asks for none: loads (the trainer restores them)
    a.load_state_dict(sd)                               # the same ones: loads
    a.load_state_dict(make().state_dict())              # a state without the keys: loads
    for key, cfg, what in SIDECAR:
        b = make()
        b.step_features[key] = dict(cfg, **{list(cfg)[1]: 0.125})
        with pytest.raises(ValueError, match=what) as e:
            b.load_state_dict(sd)
        assert "or with none: the saved one is restored), or start a new run" in str(e.value)
    # a state as the commit before the table wrote it, key by key
    old = {"format": 2, "t": 8, "lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "names": ["lin.weight"],
           "exp_avg": {"lin.weight": torch.ones(4, 6)}, "exp_avg_sq": {"lin.weight": torch.full((4, 6), 2.0)},
           "kl_schedule": dict(KL_CFG), "factor_penalty": dict(FACTOR_CFG), "smoothing_penalty": dict(SMOOTH_CFG)}
    assert set(old) == set(sd)
    c = make()
    c.step_features["factor_penalty"] = dict(FACTOR_CFG)
    c.load_state_dict(old)
    assert c.t == 8 and float(c.exp_avg.sum()) == 24.0 and float(c.exp_avg_sq.sum()) == 48.0
