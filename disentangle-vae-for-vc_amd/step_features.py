"""The opt-in features of the train step, one small object each.  The trainer keeps them in ONE ordered
table (`trainer.features`) and asks every question through it: is it on, what does it add to the graph signature, which floats
do its device scalars hold at step k, what is its backward root, what joins the epoch's sums and how is it reported, under which
key does its configuration ride in the optimiser's `.opt` sidecar.  A feature holds its own state; the trainer's setter
(`set_kl_schedule`, ...) validates and switches it."""
import torch

from . import ops


def ramp(w, n, k):
    """The linear warm-up of a weight: `w` after `n` optimiser steps (and without a warm-up), w k / n before."""
    return w if n <= 0 else w * min(1.0, k / n)


class StepFeature:
    name = None         # in the trainer's table, and of its running sum in train()'s one copy
    key = None          # of the configuration in FlatAdam.state_dict (None: not there); the trainer's setter is set_<key>
    label = None        # in messages
    lead = ()           # the configuration's entries the setter takes positionally: for a penalty the weights that ramp
    tap = None          # the model's flag that makes forward_full leave this feature's inputs
    rooted = True       # adds a backward root to the step
    rank = 0            # its place in the graph signature and in the step's one host-to-device send
    device_cofs = False     # its kernels read (mse_cof, kl_cof) from `coef`: the two are no kernel arguments of the loss

    def __init__(self, trainer):
        self.trainer = trainer
        self.cfg = None                 # a plain dict; None is "off"
        self.coef = self.aux = None     # the device scalars the kernels read, the statistics the step leaves: allocated once
        self.weights = self.sent = None     # as last computed for a step, as the device scalars hold them
        self.report = self.dims = None  # what train() left of the last epoch (dims: the KL schedule's, per latent dimension)

    @property
    def on(self):
        return self.cfg is not None

    def signature(self):
        """What being on adds to the graph signature: what changes the launches of a step (the weights are device scalars)."""
        return ((self.name,),)

    def weights_at(self, k, epoch=1):
        """The floats the device scalars hold for the step that runs after `k` optimiser steps."""
        n = int(self.cfg["warmup_steps"])
        return tuple(ramp(float(self.cfg[w]), n, k) for w in self.lead)

    def before_step(self):
        """What has to happen before a step and never inside a capture."""

    def require(self, unsplit, labels2):
        if not unsplit:
            raise RuntimeError(f"the {self.label} needs the unsplit forward (forward_full / losses_vector_full)")

    def root(self, outs, data1, data2, labels2):
        """The extra backward root of the step: ONE backward adds its gradients to the loss's (ops.FanoutFn: one sum each)."""

    def after_step(self):
        pass

    n_record = property(lambda self: self.record().numel())

    def record(self):
        """What of the step's statistics joins the epoch's running float64 sum."""
        return self.aux

    def restore(self, saved):
        """A checkpoint's configuration calls the setter again."""
        setter, saved = getattr(self.trainer, "set_" + self.key, None), dict(saved)
        if setter is not None:
            setter(*[saved.pop(k) for k in self.lead], **saved)


class KLFeature(StepFeature):
    """set_kl_schedule: no root of its own; losses_vector_full selects ops.LossGVAE2SchedFn, which reads `coef` (mse_cof, KL
    weight) and `fb` (the free bits) and leaves the per-dimension KL in `aux`."""
    name, key, label, lead, rooted, device_cofs = "kl", "kl_schedule", "KL schedule", ("kind",), False, True
    sched = fb = None

    def signature(self):
        return (("kl_sched", self.sched.free_bits is not None),)

    def weights_at(self, k, epoch=1):
        return float(self.trainer.mse_cof), float(self.sched.weight_at(k, epoch, self.trainer.kl_cof))

    def record(self):
        D = (self.aux.numel() - 4) // 4
        return self.aux[2:4 + 2 * D]       # the free counts and the per-dimension KL

    def stats(self, k, steps, weights, epoch=None):
        n, D = max(1, steps), (len(k) - 2) // 2
        z1, z2 = [v / n for v in k[2:2 + D]], [v / n for v in k[2 + D:2 + 2 * D]]
        self.dims = {"epoch": epoch, "steps": steps, "z1": z1, "z2": z2}
        return {"KL/Weight": weights[1], "KL/Free dims z1": k[0] / n, "KL/Free dims z2": k[1] / n,
                "KL/Active dims": sum(1 for v in z1 if v > 0.01)}


class FactorFeature(StepFeature):
    name, key, label, lead, tap, rank = "factor", "factor_penalty", "factor penalty", ("tc_weight", "shared_weight"), "factor_tap", 2

    def root(self, outs, data1, data2, labels2):
        # reads the aliases forward_full left of (z, q_mu, q_lv) and the two weights on the device
        m = self.trainer.model
        pen = ops.FactorPenaltyFn.apply(*m.factor_inputs, m.speaker_size, self.coef, self.aux)
        m.factor_inputs = None
        return pen

    def stats(self, f, steps, w, epoch=None):
        n = max(1, steps)
        return {"Factor/TC style": f[0] / n, "Factor/TC content": f[1] / n, "Factor/Shared": f[2] / n, "Factor/MI": f[3] / n,
                "Factor/Penalty": f[4] / n, "Factor/Weight tc": w[0], "Factor/Weight shared": w[1]}


class SmoothFeature(StepFeature):
    name, key, label, lead, tap, rank = "smooth", "smoothing_penalty", "smoothing penalty", ("ms_weight", "gv_weight"), "smooth_tap", 3

    def signature(self):
        return (("smooth", self.cfg["window"], self.cfg["floor"]),)      # both are kernel arguments

    def root(self, outs, data1, data2, labels2):
        # reads the alias forward_full left of rec_hat, the step's two inputs as its targets and the two weights on the device
        m = self.trainer.model
        pen = ops.SmoothingPenaltyFn.apply(*m.smooth_inputs, data1, data2, self.cfg["window"], self.cfg["floor"], self.coef,
                                           self.aux)
        m.smooth_inputs = None
        return pen

    def stats(self, f, steps, w, epoch=None):
        n = max(1, steps)
        return {"Smooth/MS distance dB": f[2] / n, "Smooth/GV ratio dB": f[3] / n, "Smooth/MS loss": f[0] / n,
                "Smooth/GV loss": f[1] / n, "Smooth/Penalty": f[4] / n, "Smooth/Weight ms": w[0], "Smooth/Weight gv": w[1]}


class AdvFeature(StepFeature):
    """set_speaker_adversary: `net` is the classifier (adversary.SpeakerAdversary) with an optimiser of its own; `aux` / `pred`
    are what its loss leaves of the last step.  Its checkpoint is a file of its own (`<base>.adv.pth`), not the .opt sidecar."""
    name, label, lead, rank, n_record = "adv", "speaker adversary", ("weight",), 1, 4
    net = pred = None

    def signature(self):
        return (("adv", self.net.hidden, self.net.n_speakers),)

    def before_step(self):
        # the guard of the model's optimiser covers the adversary's: a step the one skips on a non-finite gradient must not feed
        # NaNs into the other's moments.  The first set_grad_clip allocates (the model's guard is part of the graph signature, so
        # switching it captures again, after this)
        opt = self.net.optimizer
        guard = getattr(self.trainer.optimizer, "max_norm", None) is not None
        if guard != (opt.max_norm is not None):
            opt.set_grad_clip(float("inf") if guard else None, skip_nonfinite=True)
        opt.sync_scalars(1.0)           # after the first step nothing: its step() sends the same value

    def require(self, unsplit, labels2):
        if labels2 is None:
            raise ValueError("the speaker adversary is on (set_speaker_adversary): the step needs speaker_ids")
        super().require(unsplit, labels2)
        if self.trainer.reducer is not None:
            raise ValueError("the speaker adversary is not trained data parallel")
        self.net.optimizer.zero_grad()      # store-first parameters only: no launch, the written-once counts start over

    def root(self, outs, data1, data2, labels2):
        # q_mu [2 Bh, S + Cn]: the content means are its columns S .. S + Cn - 1; both launches run here, the classifier's
        # gradients land in its optimiser's buffer, and the backward adds the reversed gradient of q_mu to the loss's own
        stats = {}
        ce = self.net.loss(outs[2], labels2, self.coef, self.trainer.model.speaker_size, stats)
        self.aux, self.pred = stats["out"], stats["row_pred"]
        return ce

    def after_step(self):
        self.net.optimizer.step(grad_scale=1.0)

    def stats(self, a, steps, w, epoch=None):
        return {"Adv/CE": a[0] / a[1] if a[1] else float("nan"), "Adv/Accuracy": a[2] / a[1] if a[1] else float("nan"),
                "Adv/Weight": w[0]}


# the trainer's table, in the FIXED order of the backward roots (torch.autograd.backward and the ops.FanoutFn sums see it)
FEATURES = (KLFeature, FactorFeature, SmoothFeature, AdvFeature)
