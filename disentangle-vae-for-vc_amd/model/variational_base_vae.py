"""Training-loop surface of the reference's VariationalBaseModelVAE
(/root/reference/model/variational_base_vae.py:30-202), device-agnostic and data-parallel capable.

Kept: `step`, `train`, `run_training`, `load_last_model`, checkpoint naming
`DisentangledVAE_VCTK_{epoch}.pth` holding `model.state_dict()`.
Changed on purpose:
  * no hard-coded `.to("cuda")` (:81-82): batches go to `self.device`;
  * the 8 `.item()` host syncs of :70 become ONE device->host copy of the 8 scalars;
  * optional data parallelism: `attach_reducer()` installs ddp.GradReducer, after which `step`
    overlaps a bucketed RCCL all-reduce of the flat gradient buffer with backward;
  * TensorBoard is optional (tensorboardX is not a dependency): scalars go to `logs_path/scalars.jsonl`;
  * `estimate_trained_model` (:205-239) keeps its tensor part (eval-mode forward of one batch with train=False) and
    writes the mels as .npy (+ PNG when matplotlib is importable; librosa.display is not a dependency);
    `voice_conversion_mel` keeps its tensor part as `convert_mel`; vocoder / file I/O stay outside.
"""
from __future__ import annotations

import json
import os
from glob import glob
from pathlib import Path

import torch

from ..optim import ScalarSender
from ..step_features import FEATURES


def named_to_host(parts):
    """{name: 1-D device tensor} -> {name: list of floats}: every tensor as float64, ONE concatenation, ONE device-to-host copy,
    cut back by name."""
    flat = torch.cat([t.double() for t in parts.values()]).tolist()
    out, o = {}, 0
    for name, t in parts.items():
        out[name] = flat[o:o + t.numel()]
        o += t.numel()
    return out


def chunking_mel(melspectrogram, n_frames: int = 64, device="cuda"):
    """[80, L] (numpy or tensor) -> device tensor [L//T + 1, 80, T], tail zero-padded — the reference's chunking_mel
    (variational_base_vae.py:335-348), done by a HIP kernel."""
    from .._lib import check, lib, ptr, stream
    mel = torch.as_tensor(melspectrogram).to(device=device, dtype=torch.float32).contiguous()
    C, L = mel.shape
    n = L // n_frames + 1
    out = torch.empty((n, C, n_frames), device=mel.device, dtype=torch.float32)
    check(lib().dvae_mel_to_chunks(ptr(mel), ptr(out), C, L, n_frames, n, stream()), "dvae_mel_to_chunks")
    return out


class VariationalBaseModelVAE:
    def __init__(self, dataset, width, height, channels, latent_sz, learning_rate, device, log_interval, batch_size,
                 normalize=False, flatten=True):
        self.dataset = dataset
        self.width, self.height, self.channels = width, height, channels
        self.input_sz = (channels, width, height)
        self.latent_sz = latent_sz
        self.lr = learning_rate
        self.device = device
        self.log_interval = log_interval
        self.normalize_data = normalize
        self.flatten_data = flatten
        self.model = None       # set by subclasses
        self.optimizer = None
        self.batch_size = batch_size
        self.reducer = None     # ddp.GradReducer when data parallel
        # hipGraph replay of the whole train step: ~1 000 launches become one graph launch
        self._use_graph = False
        self._graph_ddp = True
        self._graph = None
        self._graph_sig = None
        self._graph_calls = 0
        # the opt-in features of the train step (step_features.py) by name, in the order of their backward roots: each holds its
        # configuration (None is "off"; the subclass's setters switch it), its device buffers and its epoch record
        self.features = {cls.name: cls(self) for cls in FEATURES}
        self.grad_stats = self.ema_stats = None
        self._step_k = None         # the host's count of optimizer.t (None: read it before the next step)
        self._epoch = 1             # the epoch train() is in (a schedule may look at it)
        self._sender = ScalarSender()
        self._loss_seed = None
        self._fold_before_shard = None

    def loss_function(self):
        raise NotImplementedError

    # ---- data parallel (new functionality: the reference is single-device)
    def attach_reducer(self, reducer):
        if reducer is not None and self.adversary is not None:
            raise ValueError("attach_reducer: the speaker adversary (set_speaker_adversary) is not trained data parallel: its "
                             "gradients are not reduced; switch it off first")
        sharded = reducer is not None and getattr(reducer, "mode", "all_reduce") == "rs_ag"
        if sharded and self.optimizer is not None:
            from ..ddp import refuse_sharded_clip, refuse_sharded_ema
            refuse_sharded_clip(self.optimizer)     # ValueError, and nothing attached: a shard's norm is not the gradient's
            refuse_sharded_ema(self.optimizer)      # likewise: the average needs the gathered weights
        self.reducer = reducer
        if self.optimizer is not None:
            # a sharded step (rs_ag) reads — and could clear — only this rank's slices of the gradient buffer: zero_grad
            # launches every step while such a reducer is attached; whatever the setting was before comes back with the
            # next reducer that is not sharded (or with None), so switching modes back and forth leaves no trace
            opt = self.optimizer
            if sharded:
                if self._fold_before_shard is None:
                    self._fold_before_shard = bool(opt.fold_zero_grad)
                if opt.fold_zero_grad:
                    opt.fold_zero_grad = False
                    opt._clean = False
            elif self._fold_before_shard is not None:
                if opt.fold_zero_grad != self._fold_before_shard:
                    opt.fold_zero_grad = self._fold_before_shard
                    opt._clean = False
                self._fold_before_shard = None

    def enable_graph(self, flag: bool = True, ddp=None):
        """Capture the train step into a hipGraph on its second call and replay it afterwards.  The first call runs
        eagerly (it is a real step, warms everything up and, under data parallelism, lets RCCL set up its communicator
        outside the capture).  The graph bakes host scalars into kernel arguments (loss coefficients, 1/batch_size,
        BatchNorm train/eval, shapes): `_graph_signature` is compared on every step and the graph is re-captured when
        any of them changed, so `update_kl()` or `model.eval()` take effect exactly as in the eager path.  The learning
        rate is NOT baked in: it lives in the optimizer's device state (`FlatAdam.sync_scalars`, called before every
        replay), so `optimizer.param_groups[0]['lr'] = ...` every step — a schedule — costs one 8-byte copy when the
        value changed and never a re-capture.
        `ddp`: with a reducer attached the bucketed RCCL all-reduces can be captured INSIDE the graph (ranks replay the
        same step a single GPU does).  OPT-IN (ddp=True or DVAE_DDP_GRAPH=1): no run with two or more ranks has shown
        it equal to the eager data-parallel step yet; without it a data-parallel step runs eagerly whatever `flag` says.
        A capture that fails falls back to the eager step with a warning (`graph_fallback` holds the reason)."""
        self._use_graph = flag
        self._graph_ddp = (os.environ.get("DVAE_DDP_GRAPH", "0") == "1") if ddp is None else bool(ddp)
        self.graph_fallback = None
        self._graph = None
        self._graph_sig = None
        self._graph_calls = 0

    def _graph_signature(self, data1):
        from .. import ops
        opt = self.optimizer
        on = self._features_on(ranked=True)
        # a feature whose kernels read the two loss weights from the device (a KL schedule): their values are no part of the graph
        cofs = () if any(f.device_cofs for f in on) else (float(self.mse_cof), float(self.kl_cof))
        return (tuple(data1.shape), tuple(opt.betas), float(opt.eps)) + cofs + (
                int(self.batch_size), bool(self.model.training),
                self.reducer is not None, getattr(self.reducer, "world_size", 1), ops.current_mode(),
                bool(ops.LSTM_PERSISTENT), bool(ops.deterministic())) + self._clip_signature() + self._ema_signature() \
            + sum((f.signature() for f in on), ())

    def _features_on(self, ranked=False):
        """The features that are on, in the table's order; `ranked`: in that of the graph signature and of the step's send."""
        on = [f for f in self.features.values() if f.on]
        return sorted(on, key=lambda f: f.rank) if ranked else on

    # the features' state under the names the setters' docstrings, DESIGN.md, the scripts and the suites use
    _of = lambda name, *attrs: [property(lambda self, a=a: getattr(self.features[name], a)) for a in attrs]     # noqa: E731
    kl_sched, kl_aux, kl_stats, kl_dims, _kl_coef = _of("kl", "sched", "aux", "report", "dims", "coef")
    adversary, adv_config, adv_out, adv_pred, adv_stats, _adv_coef = _of("adv", "net", "cfg", "aux", "pred", "report", "coef")
    factor_cfg, factor_aux, factor_stats, _fac_coef, factor_weights = _of("factor", "cfg", "aux", "report", "coef", "weights")
    smooth_cfg, smooth_aux, smooth_stats, _smooth_coef, smooth_weights = _of("smooth", "cfg", "aux", "report", "coef", "weights")
    kl_weight = property(lambda self: (self.features["kl"].weights or (None, None))[1])     # of (mse_cof, KL weight)
    adv_weight = property(lambda self: (self.features["adv"].weights or (None,))[0])
    del _of

    # the weights of the step that runs after `k` optimiser steps: weight min(1, k / warmup_steps) (step_features.ramp)
    smooth_weights_at = lambda self, k: self.features["smooth"].weights_at(k)       # noqa: E731  (w_ms, w_gv)
    factor_weights_at = lambda self, k: self.features["factor"].weights_at(k)       # noqa: E731  (w_tc, w_sh)
    adv_weight_at = lambda self, k: self.features["adv"].weights_at(k)[0]           # noqa: E731  the reversal weight

    def _feature_set(self, name):
        """A setter switched the feature `name` of the table on or reconfigured it: its device scalars are sent afresh, what it
        last computed and reported is forgotten, and every feature takes the optimiser's true step count at the next step (one
        read of FlatAdam.t)."""
        f = self.features[name]
        f.weights = f.sent = f.report = None
        self._step_k = None

    def _sync_step_coefs(self):
        """Host -> device copy of the weights of the step about to run (StepFeature.weights_at), for every feature that is on
        and whose weights changed since its last copy, in ONE send.  Beside optimizer.sync_scalars, never inside a capture.
        The step about to run is number `_step_k` by the host's ONE count, which starts from FlatAdam.t (one read) and is set
        right from it wherever the host reads the device anyway."""
        on = self._features_on(ranked=True)
        if not on:
            return              # the plain trainer: no read of optimizer.t (a device-to-host sync), no count
        if self._step_k is None:
            self._step_k = self.optimizer.t
        for f in on:
            f.weights = f.weights_at(self._step_k, self._epoch)
        send = [f for f in on if f.sent != f.weights]
        if send:
            # through the ring of pinned slots (optim.ScalarSender): a per-step schedule must not stall the host
            self._sender.send([(f.coef[:len(f.weights)], f.weights) for f in send])
            for f in send:
                f.sent = f.weights
        self._step_k += 1       # Adam advances t with this step (or skips it: set right at the next read of t)

    def _prepare_step(self, dev):
        """Everything of the host's that has to happen before a step and never inside a capture, in one place: _step_graph
        calls it before capture / replay, the eager step when _step_graph has not."""
        on = self._features_on()
        for f in on:
            f.before_step()                     # may allocate (the buffers of the adversary's non-finite guard)
        if any(f.rooted for f in on):
            from .. import ops
            ops.unit_seed(dev)                  # the seed of the extra roots: allocated outside the capture
        self._sync_step_coefs()

    def _adv_labels(self, speaker_ids, out=None):
        """speaker_ids [Bh] (host or device, any integer type) -> the [2 Bh] int32 device labels of the rows of q_mu (the x1
        half, then the x2 half: the same speakers); `out`: the static buffer of a captured step."""
        if speaker_ids is None:
            raise ValueError("the speaker adversary is on (set_speaker_adversary): step / step_async need speaker_ids")
        ids = torch.as_tensor(speaker_ids).view(-1).to(device=self.device, dtype=torch.int32)
        if out is None:
            return torch.cat([ids, ids])
        if out.numel() != 2 * ids.numel():
            raise ValueError(f"speaker_ids: {ids.numel()} labels for a batch of {out.numel() // 2} pairs")
        out[:ids.numel()].copy_(ids)
        out[ids.numel():].copy_(ids)
        return out

    def _clip_signature(self):
        """Gradient clipping on/off and the guard change the launches of a step; the VALUE of max_norm does not (a device
        scalar, FlatAdam.sync_scalars).  Nothing is added while it is off."""
        opt = self.optimizer
        if getattr(opt, "max_norm", None) is None:
            return ()
        return (("grad_clip", bool(opt.skip_nonfinite)),)

    def _ema_signature(self):
        """The weight average on/off changes the launches of a step; its decay and warm-up do not (device scalars).  Nothing
        is added while it is off."""
        return (("ema",),) if getattr(self.optimizer, "ema_decay", None) is not None else ()

    def ema_weights(self):
        """`with trainer.ema_weights(): ...` — forward passes, conversion and probing inside the body run on the averaged
        weights (FlatAdam.set_ema); the weights come back when it leaves.  BatchNorm running statistics are buffers, moving
        averages already, and are the same inside and outside."""
        return self.optimizer.ema_weights()

    def _eager_train_step(self, data1, data2, prepared=False, labels2=None):
        # (until round 5 the step ran inside an ops.ZeroArena: one clear launch for the outputs that split-k contractions
        # accumulated into atomically; split contractions store slabs now and nothing needs clearing)
        if not prepared:                # _step_graph has prepared the step itself, before capture / replay
            self._prepare_step(data1.device)
        return self._train_step_body(data1, data2, labels2)

    def _train_step_body(self, data1, data2, labels2=None):
        self.optimizer.zero_grad()
        rooted = [f for f in self._features_on() if f.rooted]
        unsplit = hasattr(self, "losses_vector_full") and hasattr(self.model, "forward_full")
        for f in rooted:
            f.require(unsplit, labels2)     # raises before anything is launched
        if unsplit:
            # the eight scalars as one vector (fused loss kernels) on the UNSPLIT outputs; backward is seeded with the
            # constant (1, 0, ..., 0): `vec[0].backward()` and the reference's ten output slices cost ~25 zero-fill /
            # copy launches of autograd glue per step
            outs = self.model.forward_full(data1, data2)
            vec = self.losses_vector_full(data1, data2, *outs)
            losses = None
        else:
            vec = None
            losses = self.loss_functionGVAE2(data1, data2, *self.model(data1, data2), train=True)
        if self.reducer is not None:
            self.reducer.begin()
        if vec is not None:
            if self._loss_seed is None or self._loss_seed.device != vec.device:
                self._loss_seed = torch.zeros(8, device=vec.device)
                self._loss_seed[0] = 1.0
            if rooted:
                # LOSS + the features' roots, in the table's order: ONE backward (StepFeature.root)
                from .. import ops
                torch.autograd.backward([vec] + [f.root(outs, data1, data2, labels2) for f in rooted],
                                        [self._loss_seed] + [ops.unit_seed(vec.device)] * len(rooted))
            else:
                torch.autograd.backward(vec, self._loss_seed)
        else:
            losses[0].backward()
        if self.reducer is not None:
            self.reducer.finish()
            self.reducer.step(self.optimizer)       # full Adam after an all-reduce, or the sharded step (mode "rs_ag")
        else:
            self.optimizer.step(grad_scale=1.0)
        for f in rooted:
            f.after_step()                  # the adversary's own Adam
        return vec.detach() if vec is not None else torch.stack([l.detach() for l in losses])

    def _step_graph(self, data1, data2, speaker_ids=None):
        m = self.model
        dev = data1.device
        Bh = data1.shape[0]
        S, Cn = m.speaker_size, m.latent_dim - m.speaker_size
        self._graph_calls += 1
        adv = self.adversary
        if self._graph_calls == 1:
            return self._eager_train_step(data1, data2, labels2=self._adv_labels(speaker_ids) if adv is not None else None)
        sig = self._graph_signature(data1)
        if self._graph is not None and sig != self._graph_sig:
            self._graph = None          # a baked-in scalar or the batch shape changed: capture again
        if self._graph is None:
            self._graph_sig = sig
            self._g_x1, self._g_x2 = torch.empty_like(data1), torch.empty_like(data2)
            # the two content-noise halves are views of ONE buffer: the model uses it as is (no concatenation launch)
            eps_c = torch.empty((2 * Bh, Cn), device=dev)
            self._g_eps_c = eps_c
            self._g_eps = (eps_c[:Bh], eps_c[Bh:], torch.empty((Bh, S), device=dev))
            self._g_labels2 = torch.empty(2 * Bh, device=dev, dtype=torch.int32) if adv is not None else None
        self._g_x1.copy_(data1)
        self._g_x2.copy_(data2)
        if adv is not None:
            self._adv_labels(speaker_ids, self._g_labels2)
        user_eps = m.eps_override
        if user_eps is None:               # the eager step's two draws (content [2*Bh, Cn], style [Bh, S]), same order
            self._g_eps_c.normal_()
            self._g_eps[2].normal_()
        else:
            for dst, src in zip(self._g_eps, user_eps):
                dst.copy_(src.to(dev))
        m.eps_override = self._g_eps
        # learning rate / gradient scale: device scalars, refreshed OUTSIDE the captured region
        self.optimizer.sync_scalars(1.0 / self.reducer.world_size if self.reducer is not None else 1.0)
        self._prepare_step(dev)         # likewise what the opt-in features need (nothing while they are off)
        if self._graph is not None and not getattr(self.optimizer, "_clean", True):
            # something accumulated into the gradient buffer since the last Adam launch (a manual backward between two
            # replays): a graph captured on a clean buffer holds no zero_grad launch of its own
            self.optimizer.zero_grad()
        try:
            if self._graph is None:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                # with a reducer the RCCL collectives are captured too (opt-in, see enable_graph); its watchdog thread
                # makes HIP calls of its own, hence thread-local capture checking
                # (also without a reducer while a process group exists — bench.py times the single-rank graph inside a
                # data-parallel run: RCCL's watchdog is there either way)
                import torch.distributed as _dist
                pg = _dist.is_available() and _dist.is_initialized()
                mode = {"capture_error_mode": "thread_local"} if (self.reducer is not None or pg) else {}
                if self.reducer is not None and pg:
                    # c10d's watchdog thread polls the end events of the EAGER collectives of the warm-up steps every 100 ms
                    # until it has seen them complete.  HIP refuses hipEventQuery on an event whose stream has meanwhile
                    # entered a capture (hipErrorCapturedEvent — RCCL's stream joins this capture), the watchdog rethrows
                    # and the process aborts: seen as a rare abort of the captured data-parallel step (2 of ~15 complete
                    # test-suite runs, round 6).  The device is idle here (synchronize above): give the watchdog a few
                    # periods to retire what it still holds.  (torch's own wait for pending event queries in
                    # CUDAGraph.capture_begin covers global-mode captures only.)
                    import time as _time
                    _time.sleep(0.5)
                try:
                    with torch.cuda.graph(g, **mode):
                        self._g_losses = self._eager_train_step(self._g_x1, self._g_x2, prepared=True, labels2=self._g_labels2)
                except Exception as e:      # nothing of the step has run: fall back to the eager step, for good
                    if self.reducer is None:
                        raise
                    import warnings
                    self.graph_fallback = repr(e)[:300]
                    warnings.warn("hipGraph capture of the data-parallel step failed; running eagerly: " + self.graph_fallback)
                    self._use_graph = False
                    self._graph = None
                    torch.cuda.synchronize()
                    return self._eager_train_step(self._g_x1, self._g_x2, prepared=True, labels2=self._g_labels2)
                self._graph = g
            self._graph.replay()
            if getattr(self.optimizer, "fold_zero_grad", False):
                self.optimizer._clean = True        # the replayed Adam launch cleared the ranges (host flags do not replay)
        finally:
            m.eps_override = user_eps
        return self._g_losses.clone()       # the static buffer is overwritten by the next replay

    def step_async(self, data1, data2, speaker_ids=None):
        """One TRAIN step without any host synchronisation: the 8 loss scalars come back as a device tensor, so the
        host can enqueue the next step (noise draw, input copies, graph launch) while this one runs.  `step(...,
        train=True)` is this plus one device->host copy."""
        if self._use_graph and (self.reducer is None or self._graph_ddp):
            return self._step_graph(data1, data2, speaker_ids)
        adv = self.adversary
        return self._eager_train_step(data1, data2, labels2=self._adv_labels(speaker_ids) if adv is not None else None)

    # ---- variational_base_vae.py:58-70
    def step(self, data1, data2, speaker_ids, train=False):
        if train and self._features_on():
            # the same one copy carries the optimiser's step count: the schedules' position is exactly t (a skipped step)
            vec = torch.cat([self.step_async(data1, data2, speaker_ids), self.optimizer.dev_state[0:1]]).tolist()
            self._step_k = int(vec[8])
            self._check_and_recover()
            return tuple(vec[:8])
        if train:
            out = tuple(self.step_async(data1, data2, speaker_ids).tolist())   # one D2H copy, not 8 .item() syncs
            self._check_and_recover()
            return out
        outs = self.model(data1, data2)
        losses = self.loss_functionGVAE2(data1, data2, *outs, train=train)
        return tuple(torch.stack([l.detach() for l in losses]).tolist())

    @staticmethod
    def _check_device_errors():
        """Raises if a bounded cross-workgroup wait of a persistent LSTM launch gave up since the last check (the host is
        synchronised at every call site of this)."""
        from .. import ops
        ops.lstm_pers_check()

    def _check_and_recover(self):
        try:
            self._check_device_errors()
        except Exception:
            # the Adam launches skipped their update (and their gradient clear) while the error word was set: the next
            # zero_grad must really clear
            if self.optimizer is not None and hasattr(self.optimizer, "_clean"):
                self.optimizer._clean = False
            raise

    # ---- variational_base_vae.py:74-101
    def train(self, train_loader, epoch, logging_func=print):
        self.model.train()
        # the running sums of :88-96 live on the device (fp64); the host reads them once per epoch instead of
        # stalling the queue after every step
        f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=self.device)
        tot = f64(8)
        last, steps = None, 0
        opt = self.optimizer
        clip = getattr(opt, "max_norm", None) is not None
        ema = getattr(opt, "ema_decay", None) is not None
        on = self._features_on()
        self.grad_stats = self.ema_stats = None
        for f in self.features.values():
            f.report = f.dims = None
        self._epoch = max(1, int(epoch))
        # gradient clipping on: the step's norm (optimizer.clip_state[1]) joins running sum / max tensors the same way; a
        # norm that is not finite in float32 (a skipped step, or a huge gradient that was clipped) is counted, not averaged
        if clip:
            gsum = f64(2)           # sum of the finite norms, their number
            gmax = torch.zeros(1, dtype=torch.float32, device=self.device)
            zero = torch.zeros(1, dtype=torch.float32, device=self.device)
            before = opt.clip_state[5:7].clone()
        # every feature of the step that is on: what it records of a step (StepFeature.record) joins a running float64 tensor
        # the same way, under the feature's name
        sums = {f.name: f64(f.n_record) for f in on}
        for data1, data2, speaker_ids in train_loader:
            data1 = data1.to(self.device, non_blocking=True).float()
            data2 = data2.to(self.device, non_blocking=True).float()
            speaker_ids = speaker_ids.view(-1)
            last = self.step_async(data1, data2, speaker_ids)
            steps += 1
            tot.add_(last)
            for f in on:
                sums[f.name].add_(f.record())
            if clip:
                ok = torch.isfinite(opt.clip_state[1:2])
                norm = torch.where(ok, opt.clip_state[1:2], zero)
                gsum.add_(torch.cat([norm, ok.float()]))
                torch.maximum(gmax, norm, out=gmax)
        # the epoch's ONE device-to-host copy: every running tensor that is on, by name; while a feature with a schedule is on
        # the optimiser's step count rides along and sets the host's count right
        parts = {"loss": tot, **sums}
        if clip:
            parts.update(gsum=gsum, gmax=gmax, clip_counts=opt.clip_state[5:7] - before)
        if ema:
            parts["ema"] = opt.ema_state[1:3]
        if on:
            parts["t"] = opt.dev_state[0:1]
        host = named_to_host(parts)
        tot = host["loss"]
        if "t" in host:
            self._step_k = int(host["t"][0])
        for f in on:
            w = f.weights if f.weights is not None else f.weights_at(self._step_k, self._epoch)
            f.report = f.stats(host[f.name], steps, w, epoch=epoch)
        if clip:
            g = host["gsum"]
            self.grad_stats = {"Grad/Norm mean": g[0] / max(1.0, g[1]), "Grad/Norm max": host["gmax"][0],
                               "Grad/Skipped steps": int(host["clip_counts"][0]), "Grad/Clipped steps": int(host["clip_counts"][1])}
        if ema:
            self.ema_stats = {"EMA/Updates": int(host["ema"][0]), "EMA/Weight": host["ema"][1]}
        self._check_and_recover()
        last_style = float(last[7]) if last is not None else 0.0
        if hasattr(train_loader, "dataset") and hasattr(train_loader.dataset, "shuffle_data"):
            train_loader.dataset.shuffle_data()
        n_items = len(train_loader.dataset) if hasattr(train_loader, "dataset") else len(train_loader)
        logging_func("====> Epoch: {} Average loss: {:.4f}".format(epoch, tot[0] / max(1, n_items)))
        # NB the reference returns the style KL of the LAST batch, not the total (:101)
        return tot[1], tot[2], tot[3], tot[4], tot[5], tot[6], last_style

    # ---- variational_base_vae.py:105-123 (test), per pair and per speaker
    VAL_TERMS = ("Loss", "Reconstruction Loss1", "Reconstruction Loss2", "Reconstruction Loss1 hat",
                 "Reconstruction Loss2 hat", "Z1 KL Loss", "Z2 KL Loss", "Z KL Style")
    val_seed = 0            # seed of the validation pass's private style-noise generator
    val_batch_size = None   # pairs per validation batch (None: the configured batch size)

    def validate(self, val_pairs, logging_func=print, use_ema=False):
        """The eight loss terms on a held-out pair list (data.HeldOutPairs, or anything with `batches(batch_size)` yielding
        (x1, x2, int32 speaker index) and `speaker_ids`): eval-mode forward (`train=False`: content z = mu, BatchNorm on
        running statistics, the style sampled as the reference does in eval), per-pair terms (ops.pair_metrics: the
        reference's formulas with batch_size 1), float64 sums per speaker over all batches (ops.group_sum), ONE
        device->host copy.  `len(val_pairs)` is the number of pairs.  Means are per PAIR: independent of the batching, and on a full batch exactly what the training
        scalars report.  The style noise comes from a private generator re-seeded with `val_seed` at the start of every
        pass — the same noise every epoch and for both weight sets — so the default generator, and with it every later
        training step, is left alone; so are weights, moments, BatchNorm buffers and the loaders' streams.
        use_ema: run on the averaged weights (keys `Val EMA/...`); the live weights and their derived layouts are back
        afterwards."""
        from .. import ops
        m = self.model
        names = list(val_pairs.speaker_ids)
        G, prefix = len(names), "Val EMA/" if use_ema else "Val/"
        dev = torch.device(self.device)
        S = m.speaker_size
        gen = getattr(self, "_val_gen", None)
        if gen is None or gen.device != dev:
            gen = self._val_gen = torch.Generator(device=dev)
        gen.manual_seed(int(self.val_seed))
        sums = torch.zeros((G + 1, 8), dtype=torch.float64, device=dev)
        counts = torch.zeros(2 * (G + 1), dtype=torch.int64, device=dev)       # counts | bad
        self.val_rows = rows_all = []                                           # per-pair rows of the pass, on the device
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad():
                if use_ema:
                    self.optimizer.swap_ema()
                try:
                    # the pass's style noise, one row per pair in list order: a pair's noise does not depend on its batch
                    eps_all = torch.randn((len(val_pairs), S), device=dev, dtype=torch.float32, generator=gen)
                    Bc, done = int(self.batch_size), [0]

                    def launch(a, b, spk):
                        n = a.shape[0]
                        eps = eps_all[done[0]:done[0] + n]
                        if n < Bc:
                            pad = lambda t: torch.cat([t, t.new_zeros((Bc - n,) + tuple(t.shape[1:]))])
                            a, b, eps = pad(a), pad(b), pad(eps)
                        outs = m.forward_full(a.contiguous(), b.contiguous(), train=False, eps_style=eps.contiguous())
                        rows = ops.pair_metrics(a, b, *outs, self.mse_cof, self.kl_cof)[:n]
                        ops.group_sum(rows, spk.contiguous(), sums, counts[:G + 1], counts[G + 1:])
                        rows_all.append(rows)
                        done[0] += n

                    # The launches are a function of the pair LIST, not of how the caller batched it: pair i is row i % B of
                    # forward i // B at the training step's shape (B the configured batch size; the last one padded with
                    # silent pairs whose rows are dropped).  The contraction kernels pick tiles and splits by shape, and the
                    # W_hh-resident H = 1024 recurrence adds its four k-quarters in an order that turns with the row
                    # (csrc/lstm_pers.hip, lstm_pers_fwd_x3: the owner wave of rows 4q + {0, 1} is not that of 4q + {2, 3}), so
                    # a pair's last bits depend on its shape AND its row; fixing both makes them independent of the batching.
                    held = None
                    for piece in val_pairs.batches(self.val_batch_size or Bc):
                        held = piece if held is None else tuple(torch.cat([h, p]) for h, p in zip(held, piece))
                        while held[0].shape[0] >= Bc:
                            launch(*(t[:Bc] for t in held))
                            held = tuple(t[Bc:] for t in held)
                    if held is not None and held[0].shape[0]:
                        launch(*held)
                finally:
                    if use_ema:
                        self.optimizer.swap_ema()
                        m._refresh_derived()        # packed transposes / bf16 copies: those of the live weights again
        finally:
            m.train(was_training)
        packed = torch.cat([sums.view(-1), counts.double()]).tolist()           # the pass's one copy (counts < 2^53)
        self._check_device_errors()
        tab, cnt, bad = packed[:8 * (G + 1)], packed[8 * (G + 1):9 * (G + 1)], packed[9 * (G + 1):]
        mean = lambda g: [tab[8 * g + k] / cnt[g] if cnt[g] else float("nan") for k in range(8)]
        res = {prefix + t: v for t, v in zip(self.VAL_TERMS, mean(G))}
        res[prefix + "Pairs"], res[prefix + "Non-finite pairs"] = int(cnt[G]), int(bad[G])
        res["per_speaker"] = {name: dict(zip(self.VAL_TERMS, mean(g)), **{"Pairs": int(cnt[g]), "Non-finite pairs": int(bad[g])})
                              for g, name in enumerate(names) if cnt[g] or bad[g]}
        logging_func("====> {}set loss: {:.4f} ({} pairs)".format(prefix.replace("/", " "), res[prefix + "Loss"], int(cnt[G])))
        return res

    def test(self, test_loader, epoch, logging_func=print):
        """The reference's test() (:105-123): the held-out loss of this epoch, per pair."""
        return self.validate(test_loader, logging_func)["Val/Loss"]

    # ---- variational_base_vae.py:127-149
    def load_last_model(self, checkpoints_path, logging_func=print, use_ema=False, restore_adversary=False):
        """use_ema: take the weights from `<base>.ema.pth` (the averaged weights run_training writes next to `<base>.pth`
        while FlatAdam.set_ema is on) in place of `<base>.pth`.  A `<epoch>.ema` stem is never a checkpoint candidate.
        The speaker adversary's sidecar `<base>.adv.pth` matters only to a trainer that trains: with an adversary switched on
        it is loaded (and a different or a missing one refused); with none, it is restored from the sidecar only under
        `restore_adversary` (run_training), and otherwise left alone — conversion, probing and the reports load a checkpoint
        of an adversary run exactly as they load any other."""
        name = self.model.__class__.__name__
        ids = []
        for f in glob(f"{checkpoints_path}/*.pth"):
            parts = Path(f).stem.split("_")
            if len(parts) == 3 and parts[2].isdigit():
                ids.append((int(parts[2]), f))
        if not ids:
            logging_func(f"Training {name} model from scratch...")
            return 1
        start_epoch, last = max(ids, key=lambda it: it[0])
        weights = last
        if use_ema:
            weights = last[:-4] + ".ema.pth"
            if not os.path.exists(weights):
                raise FileNotFoundError(f"{weights} is missing: the last checkpoint ({last}) was written without a weight "
                                        "average (train with --ema-decay / FlatAdam.set_ema)")
        # the speaker adversary of the run (`<base>.adv.pth`): checked before anything is loaded
        adv_path, adv_sd = last[:-4] + ".adv.pth", None
        if self.adversary is None and not restore_adversary:
            pass
        elif os.path.exists(adv_path):
            adv_sd = torch.load(adv_path, map_location="cpu")
            want = self.adv_config if self.adversary is not None else None
            if want is not None and dict(want) != dict(adv_sd["config"]):
                raise ValueError(f"{adv_path} was trained with the speaker adversary {dict(adv_sd['config'])}, this run asks "
                                 f"for {dict(want)}: resume with the same flags (or with none: the saved ones are restored), or "
                                 "start a new run")
        elif self.adversary is not None:
            raise ValueError(f"{adv_path} is missing: the last checkpoint ({last}) was written without a speaker adversary, "
                             "and one cannot join a run half way (its classifier would start untrained against a trained "
                             "encoder); start a new run")
        self.model.load_state_dict(torch.load(weights, map_location=self.device))
        if adv_sd is not None and not use_ema and hasattr(self, "set_speaker_adversary"):
            if self.adversary is None:
                cfg = dict(adv_sd["config"])
                self.set_speaker_adversary(cfg.pop("weight"), **cfg)
            self.adversary.load_state_dict(adv_sd["adversary"])
        opt = last[:-4] + ".opt"
        if os.path.exists(opt):
            sd = torch.load(opt, map_location="cpu")
            self.optimizer.load_state_dict(sd, legacy_layout=os.environ.get("DVAE_OPT_LEGACY_LAYOUT"))
            # the features the checkpoint was trained under (load_state_dict has refused a different configuration): each is
            # restored when none was asked for, and continued either way at the step count just loaded (`_step_k` below)
            for f in self.features.values():
                if not f.on and sd.get(f.key) is not None:
                    f.restore(sd[f.key])
            if sd.get("cuda_rng_state") is not None and torch.device(self.device).type == "cuda":
                g = torch.cuda.default_generators[torch.device(self.device).index or 0]
                if self.reducer is not None and self.reducer.rank > 0:
                    # the checkpoint holds rank 0's generator.  The other ranks keep THEIR seed (train.py / bench.py seed
                    # rank r with seed + 7919 r) and continue at the checkpointed Philox offset — every rank draws the
                    # same number of normals per step — instead of replaying rank 0's noise or their own from offset 0
                    seed = int(sd.get("cuda_rng_seed", g.initial_seed())) + 7919 * self.reducer.rank
                    g.manual_seed(seed)
                    if sd.get("cuda_rng_offset") is not None:
                        g.set_offset(int(sd["cuda_rng_offset"]))
                else:
                    torch.cuda.set_rng_state(sd["cuda_rng_state"], self.device)   # eps stream continues where it stopped
        self._step_k = None         # the host's count is not the loaded optimiser's: read before the next step
        logging_func(f"Loading {name} model from last checkpoint ({start_epoch})...")
        return start_epoch + 1

    def update_(self):
        pass

    # ---- variational_base_vae.py:205-239
    @torch.no_grad()
    def estimate_trained_model(self, test_loader, checkpoints_path, estimation_dir, n_show=5):
        """Load the last checkpoint, run ONE batch through the eval-mode forward (`train=False`: content z = mu,
        BatchNorm on running statistics) and store the first `n_show` original / reconstructed mels of x1 as
        `{epoch}_original_mel_{i}.npy` / `{epoch}_recons_mel_{i}.npy` (the reference stores specshow PNGs; PNGs are
        also written here when matplotlib imports).  Returns (epoch, recons_x1, recons_x2)."""
        logging_epoch = self.load_last_model(checkpoints_path, logging_func=lambda *_: None)
        was_training = self.model.training
        self.model.eval()
        os.makedirs(estimation_dir, exist_ok=True)
        # the eval-mode forward draws its style noise from the default generator: put the generator back where the checkpoint
        # recorded it, so that the epochs behind this checkpoint draw what a run resumed from it draws
        cuda = torch.device(self.device).type == "cuda"
        rng = torch.cuda.get_rng_state(self.device) if cuda else None
        try:
            # a loader with sample_batch (data.GpuPairLoader) hands out a batch WITHOUT advancing its epoch streams: under
            # data parallelism only rank 0 comes here and must not fall out of step with the other ranks' permutations
            data1, data2, _ = test_loader.sample_batch() if hasattr(test_loader, "sample_batch") else next(iter(test_loader))
            data1 = data1.to(self.device).float()
            data2 = data2.to(self.device).float()
            outs = self.model(data1, data2, train=False)
            recons_x1, recons_x2 = outs[2], outs[3]
            try:
                import matplotlib
                matplotlib.use("Agg")
                import matplotlib.pyplot as plt
            except Exception:                      # plotting is optional
                plt = None
            for i in range(min(n_show, data1.shape[0])):
                for tag, mel in (("original", data1[i]), ("recons", recons_x1[i])):
                    arr = mel.detach().cpu().numpy()
                    base = os.path.join(estimation_dir, f"{logging_epoch}_{tag}_mel_{i}")
                    import numpy as np
                    np.save(base + ".npy", arr)
                    if plt is not None:
                        plt.figure()
                        plt.title(("reconstructed" if tag == "recons" else "original") + " mel spectrogram")
                        plt.imshow(arr, origin="lower", aspect="auto")
                        plt.colorbar(format="%f")
                        plt.savefig(base + ".png")
                        plt.close()
            return logging_epoch, recons_x1, recons_x2
        finally:
            self.model.train(was_training)
            if rng is not None:
                torch.cuda.set_rng_state(rng, self.device)

    # ---- tensor part of voice_conversion_mel (variational_base_vae.py:269-301); file I/O, plots and the WaveNet
    # vocoder of the reference stay outside
    @torch.no_grad()
    def convert_mel(self, source_mel, target_mel):
        """source_mel, target_mel: [80, L] -> dict(source, recons, converted, spectral_detail), each [80, n*T].
        Content of the source, style (mean style_mu over chunks) of the target; eval-mode BatchNorm."""
        from .._lib import check, lib, ptr, stream
        m = self.model
        was_training = m.training
        m.eval()
        try:
            T, S, Cn = m.n_frames, m.speaker_size, m.latent_dim - m.speaker_size
            src = chunking_mel(source_mel, T, self.device)
            trg = chunking_mel(target_mel, T, self.device)
            n, k = src.shape[0], trg.shape[0]
            src_style, src_content = m.encode_heads(src)      # [n, 2S], [n, 2Cn] (mu | logvar)
            trg_style, _ = m.encode_heads(trg)
            z_src = torch.empty((n, S + Cn), device=src.device, dtype=torch.float32)
            z_conv = torch.empty_like(z_src)
            L = lib()
            check(L.dvae_conversion_latents(ptr(src_style), ptr(src_content), ptr(trg_style), ptr(z_src), ptr(z_conv),
                                            n, k, S, Cn, stream()), "dvae_conversion_latents")
            recons = m.decode(z_src)
            conv = m.postnet.forward_plus_input(m.decode(z_conv))

            def cat(x, clamp):
                out = torch.empty((x.shape[1], n * T), device=x.device, dtype=torch.float32)
                check(L.dvae_chunks_to_mel(ptr(x.contiguous()), ptr(out), n, x.shape[1], T, 0.0, 1.0, int(clamp),
                                           stream()), "dvae_chunks_to_mel")
                return out
            source, recons_v, conv_v = cat(src, False), cat(recons, False), cat(conv, True)
            detail = torch.empty_like(source)
            check(L.dvae_mul_div(ptr(source), ptr(recons_v), ptr(conv_v), ptr(detail), source.numel(), stream()),
                  "dvae_mul_div")
            return {"source": source, "recons": recons_v, "converted": conv_v, "spectral_detail": detail}
        finally:
            m.train(was_training)

    @torch.no_grad()
    def convert_utterances(self, sources, targets, bank=None, style_mix=1.0, recons=False, hop=None, batch=32):
        """Whole utterances through overlapped, cross-faded windows (convert.Converter.convert):
        per source a dict with "converted" [80, L], exactly L frames.  Like convert_mel it runs the weights that are in place
        (inside `with trainer.ema_weights():` the averaged ones) in eval mode and leaves `model.training` as it found it."""
        from ..convert import Converter
        was_training = self.model.training
        try:
            return Converter(self, hop=hop, batch=batch).convert(sources, targets, bank, style_mix, recons)
        finally:
            self.model.train(was_training)

    @staticmethod
    def _note_best(checkpoints_path, base, epoch, val):
        """`best.json` names the checkpoint with the lowest Val/Loss seen at any checkpoint so far (an existing file counts:
        a resumed run).  Candidates of this epoch: the last iterate and, if written, the average.  Not a .pth:
        load_last_model never sees it."""
        import math
        path = os.path.join(checkpoints_path, "best.json")
        cands = [(val["last"]["Val/Loss"], base + ".pth", False)]
        if "ema" in val and os.path.exists(os.path.join(checkpoints_path, base + ".ema.pth")):
            cands.append((val["ema"]["Val EMA/Loss"], base + ".ema.pth", True))
        cands = [c for c in cands if math.isfinite(c[0])]
        if not cands:
            return
        loss, name, ema = min(cands, key=lambda c: c[0])
        if os.path.exists(path):
            with open(path) as fp:
                old = json.load(fp)
            if old.get("Val/Loss") is not None and old["Val/Loss"] <= loss and \
                    os.path.exists(os.path.join(checkpoints_path, old.get("weights", ""))):
                return
        with open(path, "w") as fp:
            json.dump({"epoch": epoch, "weights": name, "Val/Loss": loss, "ema": ema}, fp)

    def _is_rank0(self):
        return self.reducer is None or self.reducer.rank == 0

    # ---- variational_base_vae.py:156-202
    def run_training(self, train_loader, test_loader, epochs, report_interval, sample_sz=64, reload_model=True,
                     checkpoints_path="", logs_path="", images_path="", estimation_dir="", logging_func=print,
                     start_epoch=None, val_pairs=None, val_interval=1):
        """val_pairs (data.HeldOutPairs; None: no validation, nothing below happens): every `val_interval` epochs and at every
        checkpoint epoch rank 0 runs `validate` — on the average too while FlatAdam.set_ema is on — its numbers join the
        epoch's record, `val.json` beside `logs_path` (the command line's <log_dir>) holds the per-speaker table of the last pass, and the checkpoint with the
        lowest `Val/Loss` so far (last iterate or average) is named by `<checkpoints_path>/best.json`."""
        start_epoch = self.load_last_model(checkpoints_path, logging_func, restore_adversary=True) if reload_model else 1
        if start_epoch > 1 and hasattr(train_loader, "skip_epochs"):
            # a resumed run feeds epoch e what the uninterrupted run fed it (data.GpuPairLoader: seeded streams, replayed)
            train_loader.skip_epochs(start_epoch - 1)
        run_name = "DisentangledVAE_VCTK"
        log_f = None
        if logs_path and self._is_rank0():
            os.makedirs(os.path.join(logs_path, run_name), exist_ok=True)
            log_f = open(os.path.join(logs_path, run_name, "scalars.jsonl"), "a")
        history = []
        for epoch in range(start_epoch, start_epoch + epochs):
            r1, r2, r1h, r2h, k1, k2, ks = self.train(train_loader, epoch, logging_func)
            nb = max(1, len(train_loader))
            rec = {"epoch": epoch, "Loss/Reconstruction Loss1": r1 / nb, "Loss/Reconstruction Loss2": r2 / nb,
                   "Loss/Reconstruction Loss1 hat": r1h / nb, "Loss/Reconstruction Loss2 hat": r2h / nb,
                   "Loss/Z1 KL Loss": k1 / nb, "Loss/Z2 KL Loss": k2 / nb, "Loss/Z KL Style": ks / nb}
            # what train() left of what is on: gradient clipping, the weight average (FlatAdam.set_grad_clip, set_ema) and the
            # features of the step
            for stats in (self.grad_stats, self.ema_stats, *(f.report for f in self.features.values())):
                rec.update(stats or {})
            if self.kl_stats and logs_path and self._is_rank0():
                # beside the logs directory: <log_dir>/kl_dims.json, this epoch's mean KL per latent dimension in nats
                with open(os.path.join(os.path.dirname(os.path.normpath(logs_path)), "kl_dims.json"), "w") as fp:
                    json.dump(self.kl_dims, fp, indent=1)
            ckpt_epoch = epoch % report_interval == 0 and bool(checkpoints_path)
            val = None
            if val_pairs is not None and self._is_rank0() and (epoch % max(1, int(val_interval)) == 0 or ckpt_epoch):
                quiet = lambda *_: None
                val = {"epoch": epoch, "last": self.validate(val_pairs, quiet)}
                if getattr(self.optimizer, "ema_decay", None) is not None:
                    val["ema"] = self.validate(val_pairs, quiet, use_ema=True)
                for res in (val["last"], val.get("ema", {})):
                    rec.update({k: v for k, v in res.items() if k != "per_speaker"})
                if logs_path:
                    # beside the logs directory: the command line's <log_dir>/val.json
                    with open(os.path.join(os.path.dirname(os.path.normpath(logs_path)), "val.json"), "w") as fp:
                        json.dump({"epoch": epoch, "per_speaker": val["last"]["per_speaker"],
                                   **({"per_speaker_ema": val["ema"]["per_speaker"]} if "ema" in val else {})}, fp, indent=1)
            history.append(rec)
            if self._is_rank0():
                logging_func(json.dumps(rec))
                if log_f:
                    log_f.write(json.dumps(rec) + "\n")
                    log_f.flush()
            if epoch % report_interval == 0 and checkpoints_path and self.reducer is not None \
                    and hasattr(self.reducer, "gather_moments"):
                self.reducer.gather_moments(self.optimizer)      # a collective: every rank, before rank 0 writes
            if epoch % report_interval == 0 and self._is_rank0() and checkpoints_path:
                os.makedirs(checkpoints_path, exist_ok=True)
                with torch.no_grad():
                    base = f"{checkpoints_path}/{run_name}_{epoch}"
                    torch.save(self.model.state_dict(), base + ".pth")      # reference format: weights only
                    osd = self.optimizer.state_dict()                        # added: Adam moments + step count
                    osd["cuda_rng_state"] = torch.cuda.get_rng_state(self.device)   # + the eps generator state
                    gen = torch.cuda.default_generators[torch.device(self.device).index or 0]
                    osd["cuda_rng_seed"], osd["cuda_rng_offset"] = int(gen.initial_seed()), int(gen.get_offset())
                    torch.save(osd, base + ".opt")
                    if self.adversary is not None:
                        # beside it: the speaker adversary (the .pth keeps the reference's keys)
                        torch.save({"config": dict(self.adv_config), "adversary": self.adversary.state_dict()},
                                   base + ".adv.pth")
                    if getattr(self.optimizer, "ema_decay", None) is not None:
                        # the very state_dict above with every parameter replaced by its average; buffers (BatchNorm
                        # running statistics) are the same tensors in both files
                        with self.ema_weights():
                            torch.save(self.model.state_dict(), base + ".ema.pth")
                if val is not None:
                    self._note_best(checkpoints_path, f"{run_name}_{epoch}", epoch, val)
                # variational_base_vae.py:196-201: reconstructions of one test batch from the checkpoint just written
                if estimation_dir and test_loader is not None:
                    self.estimate_trained_model(test_loader, checkpoints_path, estimation_dir)
        if log_f:
            log_f.close()
        return history
