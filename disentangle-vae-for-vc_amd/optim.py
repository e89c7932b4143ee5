"""Flat-buffer Adam: all parameters live in ONE contiguous fp32 buffer (each parameter a 16-byte
aligned view), likewise gradients and both moments, so the optimiser is a single HBM-bound HIP
launch (dvae_adam_flat_dev: 7 x 4 bytes per parameter) and a data-parallel all-reduce runs over
contiguous slices of the gradient buffer without any packing copy.

Everything that changes between steps lives ON THE DEVICE (`dev_state`: step count, bias corrections, learning rate,
gradient scale), so a captured hipGraph replays a correct step and `param_groups[0]["lr"] = ...` (a schedule) needs no
re-capture: `sync_scalars()` — called by `step()` outside a capture and by the trainer before every replay — copies the
host values over when they changed.  The same launch clears the gradient ranges `zero_grad()` covers after reading them
(the next step's zero_grad is then free), and it does NOTHING while the sticky error word of the persistent LSTM launches
is non-zero: a recurrence that gave up a bounded wait leaves garbage gradients, and weights / moments must not consume
them before the host has looked (`ops.lstm_pers_check`).

Opt-in (`set_grad_clip`): the global L2 norm of the whole gradient is clipped and a step whose gradient is not finite is
skipped, ON THE DEVICE inside the same (captured) step: one more pass over the gradient buffer (sum of squares in
float64, dvae_grad_sumsq), a one-workgroup finalize (norm, coefficient, non-finite flag: `clip_state`) and the Adam launch
reading its gradient scale from there (dvae_adam_flat_dev_clip).  `max_norm` is a device scalar like the learning rate.
This is torch.nn.utils.clip_grad_norm_ between backward() and step() of the reference (variational_base_vae.py:68-69).

Opt-in (`set_ema`): an exponential moving average of the weights, `self.ema`, a second flat buffer shaped like `flat_p`,
updated ON THE DEVICE after the Adam launch of a full step and inside the same (captured) step: a one-workgroup tick
(dvae_ema_tick: does this step count — the conditions Adam skips on — and with what weight: `ema_state`) and one sweep
(dvae_ema_update: 8 bytes read, 4 written per parameter).  `decay` is a device scalar like the learning rate.  `swap_ema()`
/ `ema_weights()` exchange weights and average IN PLACE (dvae_swap_f32): every parameter stays the view it was, the
captured graph stays valid, and every forward entry point re-derives its operand layouts from `flat_p` anyway.
New functionality: the reference keeps the last iterate only.

Replaces torch.optim.Adam(self.model.parameters(), lr) at /root/reference/model/disentangled_vae.py:304
(betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad).
"""
from __future__ import annotations

from typing import Dict, Iterable, List

import torch

from ._lib import check, lib, ptr, stream

_ALIGN = 4  # elements (16 bytes)
_PAD = 32   # the flat buffers' length is a multiple of this: any world size up to 8 cuts it into 16-byte aligned shards


class ScalarSender:
    """Host -> device copies of a few floats that must not stall the host: a per-step schedule would wait behind a pageable
    copy every step.  The values are staged in a small ring of PINNED slots (allocated on first use) and copied
    asynchronously; a slot is reused only after the event recorded behind its last copies has completed.  Not capturable:
    callers send before a capture / replay, never inside."""
    SLOTS, WIDTH = 16, 8

    def __init__(self):
        self._ring, self._done, self._i = None, [None] * self.SLOTS, 0

    def send(self, items):
        """items: [(destination: a slice of a float32 device tensor, its values)], at most WIDTH values in all: one copy per
        destination, one event behind them.  A destination that is not on a GPU is written plainly."""
        if not items[0][0].is_cuda:
            for dst, vals in items:
                dst.copy_(torch.tensor(vals, dtype=torch.float32))
            return
        if self._ring is None:
            self._ring = torch.empty(self.SLOTS, self.WIDTH, dtype=torch.float32, pin_memory=True)
        i = self._i = (self._i + 1) % self.SLOTS
        if self._done[i] is not None:
            self._done[i].synchronize()
        slot, o = self._ring[i], 0
        for dst, vals in items:
            for v in vals:
                slot[o] = v
                o += 1
            dst.copy_(slot[o - len(vals):o], non_blocking=True)
        self._done[i] = torch.cuda.Event()
        self._done[i].record()


class FlatAdam:
    def __init__(self, named_params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, layout=None):
        """layout: object with reference_layout(name, t) / storage_layout(name, t) (the model): how a tensor shaped like
        parameter `name` maps between its STORAGE here and the reference's layout (conv weights are stored packed).
        Checkpointed moments are kept in the reference's layout, so they do not depend on how parameters are stored."""
        self.layout = layout
        items = list(named_params)
        if items and not isinstance(items[0], (tuple, list)):
            items = [(f"p{i}", p) for i, p in enumerate(items)]
        self.names: List[str] = [n for n, _ in items]
        self.params: List[torch.nn.Parameter] = [p for _, p in items]
        if not self.params:
            raise ValueError("FlatAdam got an empty parameter list")
        dev = self.params[0].device
        self.offsets: Dict[str, int] = {}
        off = 0
        for n, p in items:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FlatAdam needs fp32 parameters on one device")
            self.offsets[n] = off
            off += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.n_used = off                                  # elements that belong to parameters
        off = (off + _PAD - 1) // _PAD * _PAD              # zero tail: a sharded step cuts the buffers into equal parts
        self.numel = off
        self.flat_p = torch.zeros(off, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(off, device=dev, dtype=torch.float32)
        self.exp_avg = torch.zeros(off, device=dev, dtype=torch.float32)
        self.exp_avg_sq = torch.zeros(off, device=dev, dtype=torch.float32)
        for n, p in items:
            o = self.offsets[n]
            view = self.flat_p[o:o + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = self.flat_g[o:o + p.numel()].view_as(p)
            p._dvae_flat_owned = True      # ops._grad_buf refuses to re-allocate a gradient for such a parameter
            p._dvae_owner = self           # ... and marks this optimizer's gradient buffer as written to
        self.lr, self.betas, self.eps = lr, betas, eps
        self._zero_ranges = [(0, off)]     # what zero_grad clears: everything, minus store-first parameters
        # [t, 1-b1^t, sqrt(1-b2^t), -, lr, grad_scale, -, -]
        self.dev_state = torch.zeros(8, device=dev, dtype=torch.float32)
        self._dev_scalars = None           # (lr, grad_scale) as last written to dev_state[4:6]
        self._sender = ScalarSender()      # how sync_scalars writes them
        # gradient clipping / non-finite guard (set_grad_clip): off unless asked for
        # clip_state: [max_norm, norm, coef, grad_scale * coef, skip this step, skipped steps, clipped steps, not finite]
        self.max_norm, self.skip_nonfinite = None, True
        self.clip_state, self._clip_ws = None, None
        self._dev_max_norm = None          # max_norm as last written to clip_state[0]
        # moving average of the weights (set_ema): off unless asked for
        # ema_state: [decay, updates applied, weight of the last update, warm-up, this step's update applied, -, -, -]
        self.ema_decay, self.ema_warmup = None, True
        self.ema, self.ema_state = None, None
        self._dev_ema = None               # (decay, warmup) as last written to ema_state[0], [3]
        self.ema_swapped = False           # True: flat_p holds the average and self.ema the weights (swap_ema)
        # the features of the train step the trainer runs under (step_features.py; the setters of ConvolutionalMulVAE), key in
        # state_dict() -> configuration as plain numbers: kept here because the position of a schedule or a warm-up IS the
        # step count `t`, and so that they ride in state_dict()
        self.step_features = {}
        # True: the zero_grad ranges of flat_g are known to be zero (the last Adam launch cleared them after reading and no
        # backward kernel has accumulated since: ops._grad_buf resets it) — zero_grad() is then free
        self._clean = False
        self.fold_zero_grad = True         # let the Adam launch clear them (False: zero_grad launches every time)
        self.guard_device_errors = True    # skip the update while a persistent LSTM launch's error word is set
        # torch.optim-compatible surface used by callers of the reference wrapper
        self.param_groups = [{"params": self.params, "lr": lr, "betas": betas, "eps": eps}]

    def views_intact(self) -> bool:
        base = self.flat_p.data_ptr()
        for n, p in zip(self.names, self.params):
            if p.data_ptr() != base + 4 * self.offsets[n]:
                return False
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * self.offsets[n]:
                return False
        return True

    def set_store_first(self, names):
        """Parameters whose gradient is WRITTEN (not accumulated) by exactly one launch per step
        (ops.linear_wgrad_acc(store=True)): zero_grad leaves their slices alone — the zero-fill and the read half of the
        read-modify-write of a 134 MB gradient are pure HBM traffic.  Only for parameters that get a gradient EVERY step."""
        names = set(names)
        for n, p in zip(self.names, self.params):
            p._dvae_grad_store_first = n in names
        spans = sorted((self.offsets[n], self.offsets[n] + (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN)
                       for n, p in zip(self.names, self.params) if n in names)
        out, lo = [], 0
        for a, b in spans:
            if a > lo:
                out.append((lo, a))
            lo = max(lo, b)
        if lo < self.numel:
            out.append((lo, self.numel))
        self._zero_ranges = out
        self._clean = False

    def zero_grad(self, set_to_none: bool = False):
        # gradients are accumulated by the HIP backward kernels directly into flat_g
        # a step starts here: the written-exactly-once count of the store-first gradients starts from zero, whatever an
        # abandoned attempt (a capture that failed after backward, an exception between backward and step) left behind
        for p in self.params:
            if getattr(p, "_dvae_grad_store_first", False):
                p._dvae_sf_writes = 0
        self.__dict__.get("_slab_pending", {}).clear()      # slabs of an abandoned backward pass are not this step's
        from . import ops
        if any(o is self for o in ops._fold_owners):        # ... nor is the fold a backward pass that raised never ran
            ops._fold_owners[:] = [o for o in ops._fold_owners if o is not self]
        if self._clean:
            return      # the previous step's Adam launch cleared these ranges and nothing has accumulated since
        for lo, hi in self._zero_ranges:
            if self.flat_g.is_cuda:
                check(lib().dvae_zero_f32(self.flat_g.data_ptr() + 4 * lo, hi - lo, stream()), "dvae_zero_f32")
            else:
                self.flat_g[lo:hi].zero_()
        self._clean = self.flat_g.is_cuda and not torch.cuda.is_current_stream_capturing()

    def sync_scalars(self, grad_scale: float = None):
        """Host -> device copy of (lr, grad_scale) when they changed since the last copy.  NOT capturable by design: the
        trainer calls it before capture / replay, `step()` calls it itself when the stream is not capturing."""
        lr = float(self.param_groups[0]["lr"])
        # None: whatever was last sent (1.0 before anything was).  0.0 is a scale like any other: the moments decay and the
        # parameters move by the decayed first moment
        if grad_scale is None:
            gs = float(self._dev_scalars[1]) if self._dev_scalars else 1.0
        else:
            gs = float(grad_scale)
        send = self._dev_scalars != (lr, gs)
        send_clip = self.max_norm is not None and self._dev_max_norm != self.max_norm
        send_ema = self.ema_decay is not None and self._dev_ema != (self.ema_decay, self.ema_warmup)
        items = []
        if send:
            items.append((self.dev_state[4:6], (lr, gs)))
            self._dev_scalars = (lr, gs)
        if send_clip:
            items.append((self.clip_state[0:1], (self.max_norm,)))
            self._dev_max_norm = self.max_norm
        if send_ema:            # [0] and [3] lie on either side of what the tick launch writes: 4 bytes each
            items += [(self.ema_state[0:1], (self.ema_decay,)), (self.ema_state[3:4], (float(self.ema_warmup),))]
            self._dev_ema = (self.ema_decay, self.ema_warmup)
        if items:
            self._sender.send(items)

    def set_grad_clip(self, max_norm=None, skip_nonfinite: bool = True):
        """Clip the global L2 norm of the whole gradient (grad_scale included: under data parallelism the averaged one) to
        `max_norm` before Adam reads it — torch.nn.utils.clip_grad_norm_, its 1e-6 included — and, with `skip_nonfinite`,
        skip the step whose gradient holds an inf or a NaN: weights, moments and the step count keep their bits, the
        gradient ranges are cleared all the same.  None: off, the step launches what it launched without this feature.
        float("inf"): the norm is measured and the guard is up, nothing is ever clipped.
        `max_norm` is sent to the device by sync_scalars like the learning rate: changing it between steps costs one small
        copy and no re-capture; switching the feature on or off changes the launches of a step (the trainer re-captures)."""
        if max_norm is None:
            self.max_norm = None
            return
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError(f"FlatAdam.set_grad_clip: max_norm must be positive (inf: never clip), got {max_norm}")
        if not self.flat_g.is_cuda:
            raise RuntimeError("FlatAdam.set_grad_clip: the gradient norm is computed only on the HIP device (no CPU fallback)")
        if self.clip_state is None:         # allocated once: a captured graph holds their addresses
            self.clip_state = torch.zeros(8, device=self.flat_g.device, dtype=torch.float32)
            nbytes = int(lib().dvae_grad_sumsq_ws_bytes(self.numel))
            self._clip_ws = torch.zeros(nbytes // 8, device=self.flat_g.device, dtype=torch.float64)
        self.max_norm, self.skip_nonfinite = max_norm, bool(skip_nonfinite)

    def grad_clip_stats(self):
        """What the last step's finalize left, from ONE device->host copy: norm (of the gradient Adam consumed, before
        clipping; inf above the float32 range), coef (1.0: not clipped), nonfinite (the gradient held an inf or a NaN),
        and the running counts of skipped and clipped steps."""
        if self.clip_state is None:
            raise RuntimeError("FlatAdam.grad_clip_stats: gradient clipping was never switched on (set_grad_clip)")
        c = self.clip_state.tolist()
        return {"norm": c[1], "coef": c[2], "nonfinite": int(c[7]), "skipped": int(c[5]), "clipped": int(c[6])}

    def set_ema(self, decay=None, warmup: bool = True, reset: bool = False):
        """Keep an exponential moving average of the weights in `self.ema`: after every full step that Adam applied,
        ema += w (p - ema) with w = 1 - d, d = decay, or with `warmup` d = min(decay, (1 + k) / (10 + k)) at the k-th update
        (the first updates then follow the weights instead of holding on to the initial values).  A step Adam skips (the
        non-finite guard of set_grad_clip, the error word of the persistent LSTM launches) leaves the average alone.
        The first call allocates the buffer — once: a captured graph holds its address — and starts it from the weights;
        later calls change `decay` / `warmup` only, which sync_scalars sends to the device like the learning rate: a small
        copy and no re-capture, while switching the average on or off changes the launches of a step (the trainer
        re-captures).  reset: start over from the current weights with no update counted.  None: the updates stop, the
        average stays where it is and stays usable for swap_ema / ema_weights / state_dict.
        Only parameters are averaged: BatchNorm running statistics are buffers, moving averages already, and not touched."""
        if decay is None:
            self.ema_decay = None
            return
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"FlatAdam.set_ema: decay must be in [0, 1), got {decay}")
        if not self.flat_p.is_cuda:
            raise RuntimeError("FlatAdam.set_ema: the average is kept only on the HIP device (no CPU fallback)")
        if self.ema is None:                # allocated once: a captured graph holds their addresses
            self.ema = torch.empty_like(self.flat_p)
            self.ema_state = torch.zeros(8, device=self.flat_p.device, dtype=torch.float32)
            reset = True
        if reset:
            if self.ema_swapped:
                raise RuntimeError("FlatAdam.set_ema(reset=True) while the average is swapped in (swap_ema): flat_p holds "
                                   "the average, not the weights")
            self.ema.copy_(self.flat_p)
            self.ema_state[1:3].zero_()
            self.ema_state[4:5].zero_()
        self.ema_decay, self.ema_warmup = decay, bool(warmup)

    def _need_ema(self, what):
        if self.ema is None:
            raise RuntimeError(f"FlatAdam.{what}: the weight average was never switched on (set_ema)")

    def ema_stats(self):
        """What the last step's tick left, from ONE device->host copy: the updates applied so far, the weight 1 - d of the
        last one, the decay the device holds, and whether the last step's update was applied (1) or skipped (0)."""
        self._need_ema("ema_stats")
        c = self.ema_state.tolist()
        return {"updates": int(c[1]), "weight": c[2], "decay": c[0], "applied": int(c[4])}

    def swap_ema(self):
        """Exchange the weights and their average in place: afterwards every parameter (a view of flat_p) reads the
        average, and `self.ema` holds the weights until the next call swaps them back.  step() refuses while swapped."""
        self._need_ema("swap_ema")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FlatAdam.swap_ema: not inside a graph capture")
        check(lib().dvae_swap_f32(ptr(self.flat_p), ptr(self.ema), self.numel, stream()), "dvae_swap_f32")
        self.ema_swapped = not self.ema_swapped

    def ema_weights(self):
        """`with opt.ema_weights(): ...` — the body sees the averaged weights; the weights come back when it leaves, also
        through an exception."""
        import contextlib

        @contextlib.contextmanager
        def swapped():
            self.swap_ema()
            try:
                yield self
            finally:
                self.swap_ema()
        return swapped()

    def _ema_views(self):
        """the average per parameter, whichever side of a swap it is on"""
        return self._moment_views(self.flat_p if self.ema_swapped else self.ema)

    def _store_first_guard(self):
        """A store-first parameter is excluded from zero_grad: its gradient must have been WRITTEN exactly once since the
        last step (ops.LinearFn.backward counts), else Adam would consume a stale or a partial gradient."""
        bad = None
        for n, p in zip(self.names, self.params):
            if getattr(p, "_dvae_grad_store_first", False):
                w = getattr(p, "_dvae_sf_writes", None)
                if w is not None and w != 1 and bad is None:
                    bad = (n, w)
                p._dvae_sf_writes = 0
        if bad is not None:
            raise RuntimeError(f"FlatAdam: store-first gradient of {bad[0]} was written {bad[1]} times since the last step "
                               "(exactly one backward pass per step; for gradient accumulation clear the flag with "
                               "set_store_first(()) first)")

    def step(self, grad_scale: float = 1.0):
        """One Adam step over all parameters: one launch."""
        self.step_range(0, self.numel, grad_scale, tick=True)

    def step_range(self, lo: int, hi: int, grad_scale: float = 1.0, tick: bool = True):
        """The update of elements [lo, hi) of the flat buffers.  `tick` advances the step counter first: exactly one call
        per step has it set (the first).  A sharded optimizer (ddp.GradReducer(mode="rs_ag")) calls this once per bucket
        on the slice this rank owns."""
        if not self.flat_p.is_cuda:
            raise RuntimeError("FlatAdam.step runs only on the HIP device (no CPU fallback)")
        from . import ops
        from ._lib import Ranges
        import ctypes as C
        if lo % 4 or hi % 4 or not 0 <= lo < hi <= self.numel:
            raise ValueError(f"FlatAdam.step_range: [{lo}, {hi}) is not a 16-byte aligned range of the flat buffers")
        if self.ema_swapped:
            raise RuntimeError("FlatAdam.step while the weight average is swapped in (swap_ema / ema_weights): Adam would "
                               "move the average and average the weights; swap back first")
        if tick:
            if not self.views_intact():
                # model.zero_grad() (set_to_none), .to()/.float() or `p.grad = None` would detach parameters from the flat
                # buffers: the kernels would then accumulate elsewhere while Adam and the all-reduce read stale zeros
                raise RuntimeError("FlatAdam: a parameter or its .grad is no longer a view of the flat buffers "
                                   "(use optimizer.zero_grad(), never model.zero_grad()/p.grad = None/model.to())")
            self._store_first_guard()
            ops.join_side()     # weight-gradient work may still be running on the side stream
            ops.fold_pending(self)      # the k-split slabs of this step's weight gradients: one table-driven launch, fixed order
            if torch.cuda.is_current_stream_capturing():
                if self._dev_scalars is None or (grad_scale is not None and self._dev_scalars[1] != float(grad_scale)):
                    raise RuntimeError("FlatAdam.step under capture: call sync_scalars(grad_scale) before the capture")
                if self.max_norm is not None and self._dev_max_norm != self.max_norm:
                    raise RuntimeError("FlatAdam.step under capture: call sync_scalars(grad_scale) before the capture "
                                       "(max_norm changed since it was last sent)")
                if self.ema_decay is not None and self._dev_ema != (self.ema_decay, self.ema_warmup):
                    raise RuntimeError("FlatAdam.step under capture: call sync_scalars(grad_scale) before the capture "
                                       "(the EMA decay changed since it was last sent)")
            else:
                self.sync_scalars(grad_scale)
        skip = None
        if self.guard_device_errors and ops.LSTM_PERSISTENT:
            skip = lib().dvae_lstm_pers_err_word(ptr(ops.lstm_pers_workspace(self.flat_p.device)))
        rg = Ranges()
        if self.fold_zero_grad:
            spans = [(max(a, lo) - lo, min(b, hi) - lo) for a, b in self._zero_ranges if min(b, hi) > max(a, lo)]
            if len(spans) > 8:
                raise RuntimeError("FlatAdam: more than 8 zero_grad ranges")
            rg.n = len(spans)
            for i, (a, b) in enumerate(spans):
                rg.lo[i], rg.hi[i] = a, b
        o = 4 * lo
        if self.max_norm is None:
            check(lib().dvae_adam_flat_dev(self.flat_p.data_ptr() + o, self.flat_g.data_ptr() + o, self.exp_avg.data_ptr() + o,
                                           self.exp_avg_sq.data_ptr() + o, hi - lo, self.betas[0], self.betas[1], self.eps,
                                           ptr(self.dev_state), skip, C.byref(rg), int(tick), stream()), "dvae_adam_flat_dev")
        else:
            if tick:
                # the norm of the WHOLE gradient, complete since the fold above: sum of squares, then norm / coefficient /
                # non-finite flag into clip_state, which the Adam launches of this step (this one and tick=False ones) read
                check(lib().dvae_grad_sumsq(ptr(self.flat_g), self.numel, ptr(self._clip_ws), stream()), "dvae_grad_sumsq")
                check(lib().dvae_grad_clip_finalize(ptr(self._clip_ws), self.numel, ptr(self.dev_state), ptr(self.clip_state),
                                                    skip, int(self.skip_nonfinite), stream()), "dvae_grad_clip_finalize")
            check(lib().dvae_adam_flat_dev_clip(self.flat_p.data_ptr() + o, self.flat_g.data_ptr() + o,
                                                self.exp_avg.data_ptr() + o, self.exp_avg_sq.data_ptr() + o, hi - lo,
                                                self.betas[0], self.betas[1], self.eps, ptr(self.dev_state), skip,
                                                C.byref(rg), int(tick), ptr(self.clip_state), stream()),
                  "dvae_adam_flat_dev_clip")
        if self.ema_decay is not None and tick and lo == 0 and hi == self.numel:
            # a full step only: a partial range (a sharded optimizer's) never moves the average
            check(lib().dvae_ema_tick(ptr(self.ema_state), skip, ptr(self.clip_state) if self.max_norm is not None else None,
                                      stream()), "dvae_ema_tick")
            check(lib().dvae_ema_update(ptr(self.ema), ptr(self.flat_p), self.numel, ptr(self.ema_state), stream()),
                  "dvae_ema_update")
        # the whole buffer was read and cleared only by a full step; a sharded step leaves the other ranks' slices
        # untouched, and says so itself (GradReducer.step)
        self._clean = bool(self.fold_zero_grad) and lo == 0 and hi == self.numel

    @property
    def t(self) -> int:
        """Number of optimiser steps taken (kept on the device so a captured graph can advance it)."""
        return int(self.dev_state[0].item())

    STATE_FORMAT = 2      # 2: moments per parameter, in the REFERENCE's tensor layout (1 / absent: raw flat vectors)

    def _moment_views(self, flat):
        for n, p in zip(self.names, self.params):
            o = self.offsets[n]
            yield n, flat[o:o + p.numel()].view_as(p)

    def _to_ref(self, name, t):
        return self.layout.reference_layout(name, t) if self.layout is not None else t

    def _from_ref(self, name, t):
        return self.layout.storage_layout(name, t) if self.layout is not None else t

    def state_dict(self):
        """Moments per parameter in the reference's layout (what torch.optim.Adam would hold for the reference model):
        independent of the packed conv-weight storage and of the order of the flat buffer."""
        sd = {"format": self.STATE_FORMAT, "t": self.t, "lr": self.param_groups[0]["lr"], "betas": self.betas,
              "eps": self.eps, "names": list(self.names),
              "exp_avg": {n: self._to_ref(n, v).detach().cpu().contiguous() for n, v in self._moment_views(self.exp_avg)},
              "exp_avg_sq": {n: self._to_ref(n, v).detach().cpu().contiguous()
                             for n, v in self._moment_views(self.exp_avg_sq)}}
        if self.ema is not None:            # configured (set_ema), running or stopped: the average, like the moments
            st = self.ema_stats()
            sd["ema"] = {"decay": self.ema_decay if self.ema_decay is not None else st["decay"], "warmup": self.ema_warmup,
                         "updates": st["updates"],
                         "avg": {n: self._to_ref(n, v).detach().cpu().contiguous() for n, v in self._ema_views()}}
        sd.update((key, dict(cfg)) for key, cfg in self.step_features.items())
        return sd

    def load_state_dict(self, sd, legacy_layout=None):
        """legacy_layout: only for format-1 files (see below): "packed" | "torch"."""
        if sorted(sd["names"]) != sorted(self.names):
            raise ValueError("optimizer state was saved for a different set of parameters")
        for key, mine in self.step_features.items():
            saved = sd.get(key)
            if saved is not None and dict(saved) != dict(mine):
                what = key.replace("_", " ").replace("kl ", "KL ")      # "KL schedule", "factor penalty", "smoothing penalty"
                raise ValueError(f"optimizer state was trained under the {what} {dict(saved)}, this run asks for {dict(mine)}: "
                                 f"resume with the same {what.split()[-1]} (or with none: the saved one is restored), or start "
                                 "a new run")
        fmt = int(sd.get("format", 1))
        if fmt == 1:
            # raw flat vectors in the order of ITS `names`.  Two builds wrote this format and nothing in the file tells
            # them apart: before conv weights were stored packed every slice was in torch's layout [Cout][Cin][5]; the
            # build right before format 2 already stored (and saved) conv slices packed [5][Cout][Cin].  Guessing would
            # silently scramble every conv moment, so the caller has to say which one it is.
            if list(sd["names"]) != self.names:
                raise ValueError("format-1 optimizer state needs the parameter order it was saved with")
            if legacy_layout not in ("packed", "torch"):
                differs = [n for n, p in zip(self.names, self.params) if tuple(self._to_ref(n, p).shape) != tuple(p.shape)]
                if differs:
                    raise ValueError("format-1 optimizer state does not record how conv-weight slices are laid out: pass "
                                     "legacy_layout='packed' (files written by the build that stored conv weights "
                                     "[5][Cout][Cin]) or 'torch' ([Cout][Cin][5]); env DVAE_OPT_LEGACY_LAYOUT for "
                                     f"load_last_model.  Affected: {differs[:3]} ...")
            per = {}
            for key in ("exp_avg", "exp_avg_sq"):
                flat, d = sd[key], {}
                for n, p in zip(self.names, self.params):
                    o = self.offsets[n]
                    sl = flat[o:o + p.numel()]
                    if legacy_layout == "packed":
                        d[n] = self._to_ref(n, sl.view_as(p))          # slice in STORAGE layout -> reference layout
                    else:
                        d[n] = sl.view(tuple(self._to_ref(n, p).shape))
                per[key] = d
        elif fmt == self.STATE_FORMAT:
            per = {"exp_avg": sd["exp_avg"], "exp_avg_sq": sd["exp_avg_sq"]}
        else:
            raise ValueError(f"optimizer state format {fmt} is newer than this build understands ({self.STATE_FORMAT})")
        self.dev_state.zero_()
        self.dev_state[0] = float(sd["t"])
        self._dev_scalars = None           # lr / grad_scale are re-sent by the next sync_scalars
        self.param_groups[0]["lr"] = float(sd["lr"])
        for key, flat in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for n, v in self._moment_views(flat):
                src = per[key][n]
                want = tuple(self._to_ref(n, v).shape)
                if tuple(src.shape) != want:
                    raise ValueError(f"optimizer state of {n}: shape {tuple(src.shape)}, expected {want}")
                v.copy_(self._from_ref(n, src.to(v.device)))
        if self.ema is not None:
            # the average continues from the file when it has one (the decay stays the caller's); else it starts from the
            # weights as they are now — load the model's weights first — with no update counted
            if self.ema_swapped:
                raise RuntimeError("FlatAdam.load_state_dict while the weight average is swapped in (swap_ema)")
            saved = sd.get("ema")
            if saved is None:
                self.ema.copy_(self.flat_p)
                updates = 0.0
            else:
                for n, v in self._moment_views(self.ema):
                    src = saved["avg"][n]
                    want = tuple(self._to_ref(n, v).shape)
                    if tuple(src.shape) != want:
                        raise ValueError(f"optimizer state, average of {n}: shape {tuple(src.shape)}, expected {want}")
                    v.copy_(self._from_ref(n, src.to(v.device)))
                updates = float(saved["updates"])
            self.ema_state[1:3].zero_()
            self.ema_state[4:5].zero_()
            self.ema_state[1] = updates
