"""Speaker adversary on the content latent: a speaker classifier Linear(dim, hidden) -> ReLU ->
Linear(hidden, n_speakers) trained on the content means of every training step, whose gradient reaches the encoder REVERSED
and scaled by a weight lambda (Ganin & Lempitsky 2015; Chou et al. 2018 for voice conversion).  The reference has such a
classifier with a cross-entropy loss (model/feature_selection.py:5-43) but never trains the encoder against it.

    lambda = 0     a live leakage monitor: the classifier learns, the model's step is untouched
    lambda > 0     the encoder is pushed to make the classifier fail: speaker identity leaves the content block

The whole of it — forward, loss, both backward passes — is two HIP launches (ops.SpeakerAdversaryFn: dvae_adv_rows,
dvae_adv_params, csrc/adversary.hip) plus the classifier's own Adam launch, all inside the trainer's replayed graph
(ConvolutionalMulVAE.set_speaker_adversary).  GPU only, no CPU fallback.
"""
from __future__ import annotations

import math

import torch

_B2_PAD = 32      # b2 is stored with this granularity: the four parameters then fill the optimiser's flat buffers exactly


def pad_dim(n: int) -> int:
    """the classifier's input width rounded up to 16-byte rows of w1 (4 floats)"""
    return (int(n) + 3) // 4 * 4


class SpeakerAdversary:
    """The classifier's four parameters and an optim.FlatAdam of their own.  w1 [hidden, pad_dim(dim)] (padding columns
    zero), b1 [hidden], w2 [n_speakers, hidden], b2 [n_speakers rounded up to 32] (padding zero).  Initialisation: nn.Linear's
    default (U(+-1 / sqrt(fan_in)) for weight and bias) drawn from a CPU generator seeded with `seed`, as probe.SpeakerProbe
    does.  Every parameter is store-first: dvae_adv_params STORES the whole gradient every step, so the optimiser never
    launches a zero-fill, and nothing ever writes the padding's gradient, which stays the zero it was allocated as — the padding
    stays zero."""

    def __init__(self, dim: int, n_speakers: int, hidden: int = 256, seed: int = 0, device="cuda", lr: float = 1e-3):
        from . import ops
        from .optim import FlatAdam
        dim, n_speakers, hidden = int(dim), int(n_speakers), int(hidden)
        if not 1 <= dim <= ops.ADV_MAX_D:
            raise ValueError(f"SpeakerAdversary: dim {dim}; the kernels take 1 .. {ops.ADV_MAX_D}")
        if not 1 <= n_speakers <= ops.CE_MAX_CLASSES:
            raise ValueError(f"SpeakerAdversary: {n_speakers} speakers; the kernels take 1 .. {ops.CE_MAX_CLASSES}")
        if hidden % 64 or not 64 <= hidden <= ops.ADV_MAX_H:
            raise ValueError(f"SpeakerAdversary: hidden {hidden}; a multiple of 64 in 64 .. {ops.ADV_MAX_H}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("SpeakerAdversary runs on the HIP path only (no CPU fallback)")
        self.dim, self.n_speakers, self.hidden, self.seed, self.lr = dim, n_speakers, hidden, int(seed), float(lr)
        self.dim_p = pad_dim(dim)
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seed)

        def draw(rows, cols, cols_p, rows_p, fan_in):
            b = 1.0 / math.sqrt(fan_in)
            w = torch.zeros(rows, cols_p)
            w[:, :cols] = torch.empty(rows, cols).uniform_(-b, b, generator=g)
            bias = torch.zeros(rows_p)
            bias[:rows] = torch.empty(rows).uniform_(-b, b, generator=g)
            return w, bias

        w1, b1 = draw(hidden, dim, self.dim_p, hidden, dim)
        w2, b2 = draw(n_speakers, hidden, hidden, (n_speakers + _B2_PAD - 1) // _B2_PAD * _B2_PAD, hidden)
        self.params = {k: torch.nn.Parameter(v.to(self.device)) for k, v in (("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2))}
        self.optimizer = FlatAdam(list(self.params.items()), lr=self.lr)
        self.optimizer.set_store_first(list(self.params))
        assert self.optimizer._zero_ranges == [], self.optimizer._zero_ranges
        self._zero_coef = torch.zeros(1, device=self.device, dtype=torch.float32)      # evaluate: no reversal weight

    def config(self) -> dict:
        return dict(dim=self.dim, n_speakers=self.n_speakers, hidden=self.hidden, seed=self.seed)

    def loss(self, q_mu, labels, coef, col0=0, stats=None):
        """ops.SpeakerAdversaryFn on the columns [col0, col0 + dim) of q_mu: the cross-entropy (a device scalar whose
        backward hands q_mu the reversed gradient), with the classifier's gradients left in its optimiser's buffer."""
        from .ops import SpeakerAdversaryFn
        p = self.params
        return SpeakerAdversaryFn.apply(q_mu, labels, p["w1"], p["b1"], p["w2"], p["b2"], coef, col0, self.dim, stats)

    def evaluate(self, q_mu, labels) -> dict:
        """q_mu [n, dim] content means, labels [n] (negative: ignored) -> {loss, accuracy, n} over the counted rows.  No
        gradient is computed or stored."""
        from .ops import speaker_adversary
        q = torch.as_tensor(q_mu).to(device=self.device, dtype=torch.float32).contiguous()
        y = torch.as_tensor(labels).to(device=self.device, dtype=torch.int32).contiguous().view(-1)
        if q.dim() != 2 or q.shape[1] != self.dim or y.numel() != q.shape[0]:
            raise ValueError(f"SpeakerAdversary.evaluate: q_mu [n, {self.dim}] with one label per row")
        p = self.params
        with torch.no_grad():
            out = speaker_adversary(q, y, p["w1"].detach(), p["b1"].detach(), p["w2"].detach(), p["b2"].detach(),
                                    self._zero_coef, 0, self.dim, None)[0]
        s, n, k, _ = out.tolist()
        return dict(loss=s / n if n else float("nan"), accuracy=k / n if n else float("nan"), n=int(n))

    def state_dict(self) -> dict:
        return {"config": self.config(), "params": {k: v.detach().cpu().clone() for k, v in self.params.items()},
                "optimizer": self.optimizer.state_dict()}

    def load_state_dict(self, sd):
        if dict(sd["config"]) != self.config():
            raise ValueError(f"speaker adversary state was saved for {dict(sd['config'])}, this one is {self.config()}")
        for k, v in self.params.items():
            src = sd["params"][k]
            if tuple(src.shape) != tuple(v.shape):
                raise ValueError(f"speaker adversary state, {k}: shape {tuple(src.shape)}, expected {tuple(v.shape)}")
        with torch.no_grad():
            for k, v in self.params.items():
                v.copy_(sd["params"][k].to(self.device))
        self.optimizer.load_state_dict(sd["optimizer"])
