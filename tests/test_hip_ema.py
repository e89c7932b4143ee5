"""The exponential moving average of the weights on the MI355X (csrc/elem.hip: ema_tick_kernel, ema_update_kernel,
swap_kernel; optim.FlatAdam.set_ema / swap_ema / ema_weights; the trainer's checkpoints and the command line) against the
float64 reference of tests/ema_ref.py.

The bound is the one derived there: |e' - ref| <= 2^-24 (w |p - e| (1 + 2^-24) + |ref|) + the reference's own float64
roundings + 2^-126, against the float64 update fed the kernel's OWN float32 w; the tick's w is held to 2^-23 relative on its
own, so the two checks compose and neither hides the other.  Exact properties are asserted on the bits: a repeated launch, an
element with p == e, a skipped step, the exchange.  Sizes reach every path of the sweep: one float4, either side of one
workgroup trip (256 threads x 2 float4), and a few float4 past one full sweep of the capped grid (2048 workgroups), where the
grid-stride loop makes a second, ragged trip.  The average and ema_state lie in guarded buffers (tests/kernel_harness.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import bits, Buf, DEV, child, dev_equal, down, flat, EINVAL, guards, make_trainer, same_bits
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib  # noqa: E402
from dvae_amd.optim import FlatAdam  # noqa: E402
from adam_ref import LR, grad_mixture, params  # noqa: E402
from ema_ref import TICK_REL, update_bounds, weight_at, worst_ratio  # noqa: E402

U, CAP = 2, 2048                              # EMA_U and the grid cap of csrc/elem.hip
TRIP = 4 * 256 * U                            # elements one workgroup handles per trip
SWEEP = CAP * TRIP                            # ... and the whole capped grid: 4 194 304
SIZES = [4, TRIP - 4, TRIP, TRIP + 4, SWEEP + 4 * 259]      # the last: 256 threads with a first float4, 3 with a second
RESERVED = (11.0, 12.0, 13.0)                 # ema_state[5:8]: never written


# ------------------------------------------------------------------ the three new launches through ctypes
class Ema:
    """p, the average and ema_state on the device, the latter two in guarded buffers, 32 bytes behind a multiple of 256."""

    def __init__(self, e, p, decay, warmup, k=0, w=0.0, applied=0.0):
        self.n = int(np.size(e))
        self.e = Buf(data=np.array(e, np.float32).reshape(-1), lead=32)
        self.p = torch.tensor(np.asarray(p, np.float32), device=DEV)
        self.p0 = self.p.clone()
        self.st = Buf(data=np.array([decay, k, w, float(warmup), applied, *RESERVED], np.float32), lead=32)
        self.e_ptr, self.st_ptr = self.e.ptr, self.st.ptr

    def tick(self, skip=None, clip=None):
        assert _lib.lib().dvae_ema_tick(self.st_ptr, None if skip is None else skip.data_ptr(),
                                        None if clip is None else clip.data_ptr(), _lib.stream()) == 0

    def update(self):
        assert _lib.lib().dvae_ema_update(self.e_ptr, self.p.data_ptr(), self.n, self.st_ptr, _lib.stream()) == 0

    def read(self):
        torch.cuda.synchronize()
        assert dev_equal(self.p, self.p0), "p was written"
        guards(self.e, self.st)
        e, st = self.e.np(), self.st.np()
        assert tuple(st[5:8]) == RESERVED, "a reserved word of ema_state was written"
        return e, st


@pytest.fixture(scope="module")
def draws():
    """Per size an average and two sets of weights, shared by the tests below and left unchanged: `near` is one optimiser step
    away (the average plus 1e-3 x the gradient mixture: from bit-equal to a unit apart), `far` is an independent draw."""
    out = {}
    for n in SIZES:
        e = params(n % 991, n)
        near = (e.astype(np.float64) + 1e-3 * grad_mixture(n % 997, n).astype(np.float64)).astype(np.float32)
        far = params(n % 983 + 1000, n)
        for a in (e, near, far):
            a.setflags(write=False)
        out[n] = {"e": e, "near": near, "far": far}
    return out


@pytest.mark.parametrize("kind", ["near", "far"])
@pytest.mark.parametrize("n", SIZES)
def test_update_against_float64_and_bit_identical_twice(draws, n, kind):
    e0, p = draws[n]["e"], draws[n][kind]
    k0 = 3 if kind == "near" else 40              # warm-up: the 4th update is on the ramp (d = 5/14), the 41st at the decay
    runs = []
    for _ in range(2):
        c = Ema(e0, p, 0.75, True, k=k0)
        c.tick()
        c.update()
        runs.append(c.read())
    (e1, st), (e2, st2) = runs
    assert same_bits(e1, e2) and same_bits(st, st2)                       # the same state, the same bits
    assert st[1] == k0 + 1 and st[4] == 1.0 and st[0] == np.float32(0.75) and st[3] == 1.0
    w_ref = weight_at(0.75, k0 + 1, True)
    assert abs(float(st[2]) - w_ref) <= TICK_REL * w_ref
    b = update_bounds(e0, p, st[2])                                       # the kernel's own float32 w
    r, i = worst_ratio(e1, b["ref"], b["tol"])
    print(f"n={n} {kind}: w {st[2]!r}, worst error / bound = {r:.3f} at [{i}] (got {e1[i]!r}, reference {b['ref'][i]!r})")
    assert r <= 1.0
    equal = bits(e0) == bits(p)
    assert same_bits(e1[equal], e0[equal])                                # p == e bit for bit: the bits stay
    if n > 4:                                                             # (four draws may all be equal, or none)
        assert (kind == "far" or equal.any()) and not same_bits(e1[~equal], e0[~equal])       # ... and the rest did move


@pytest.mark.parametrize("w", [1.0, 0.5, 0.1, 1e-4])
def test_equal_elements_keep_their_bits(w):
    vals = np.array([0.0, 1.0, -1.0, 0.1, -0.3, 3e38, -3e38, 1e-38, 1e-40, -1e-44, 1.17549435e-38, 1.0 + 2.0 ** -23],
                    dtype=np.float32)
    e = np.resize(vals, TRIP + 4)
    c = Ema(e, e.copy(), 1.0 - w, False, k=5, w=w, applied=1.0)           # as the tick left it: no tick here
    c.update()
    got, st = c.read()
    assert same_bits(got, e)
    assert same_bits(st, np.array([np.float32(1.0 - w), 5, w, 0, 1, *RESERVED], np.float32))      # the sweep only reads it


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warm-up"])
@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_tick_over_ten_steps(decay, warmup):
    c = Ema(np.zeros(4, np.float32), np.ones(4, np.float32), decay, warmup)
    for step in range(1, 11):
        c.tick()
        st = c.read()[1]
        w_ref = weight_at(decay, step, warmup)
        assert st[1] == step and st[4] == 1.0, (step, st)
        assert abs(float(st[2]) - w_ref) <= TICK_REL * w_ref, (step, st[2], w_ref)
        assert st[0] == np.float32(decay) and st[3] == float(warmup)     # the host's words: not written
    if warmup:
        assert abs(float(st[2]) - (1.0 - min(float(np.float32(decay)), 11.0 / 20.0))) <= TICK_REL


@pytest.mark.parametrize("how", ["error_word", "clip_flag"])
def test_skipped_step_keeps_every_bit_and_the_next_continues(draws, how):
    n = TRIP + 4
    e0, p = draws[n]["e"], draws[n]["far"]
    c = Ema(e0, p, 0.9, True)
    for _ in range(3):
        c.tick()
        c.update()
    e3, st3 = c.read()
    assert st3[1] == 3 and st3[4] == 1.0
    word = torch.tensor([2, 0, 0, 0], dtype=torch.uint8, device=DEV)      # a uint32 holding 2
    clip = torch.zeros(8, dtype=torch.float32, device=DEV)
    if how == "error_word":
        c.tick(skip=word, clip=clip)
    else:
        clip[4] = 1.0
        c.tick(skip=word.zero_(), clip=clip)
    c.update()
    e4, st4 = c.read()
    assert same_bits(e4, e3), "a skipped step moved the average"
    assert st4[4] == 0.0 and same_bits(st4[:4], st3[:4])                  # applied <- 0; k, w, decay, warm-up keep their bits
    word.zero_()
    clip.zero_()
    c.tick(skip=word, clip=clip)                                          # both given, both clear: applied
    c.update()
    e5, st5 = c.read()
    assert st5[1] == 4 and st5[4] == 1.0 and abs(float(st5[2]) - weight_at(0.9, 4, True)) <= TICK_REL
    b = update_bounds(e3, p, st5[2])
    assert worst_ratio(e5, b["ref"], b["tol"])[0] <= 1.0 and not same_bits(e5, e3)


def test_bad_arguments_are_refused_without_touching_memory(draws):
    n = TRIP
    c = Ema(draws[n]["e"], draws[n]["far"], 0.9, True, k=2, w=0.25, applied=1.0)
    L, st = _lib.lib(), _lib.stream()
    e, p, s = c.e_ptr, c.p.data_ptr(), c.st_ptr
    assert L.dvae_ema_tick(None, None, None, st) == EINVAL
    for args in ((None, p, n, s), (e, None, n, s), (e, p, n, None), (e, p, 0, s), (e, p, 6, s), (e, p, -4, s),
                 (e + 4, p, n - 4, s), (e, p + 4, n - 4, s), (e, e + 16, 8, s), (e + 16, e, 8, s), (e, e, n, s)):
        assert L.dvae_ema_update(*args, st) == EINVAL, args
    for args in ((None, p, n), (e, None, n), (e, p, 0), (e, p, 6), (e + 4, p, n - 4), (e, p + 4, n - 4), (e, e + 16, 8),
                 (e, e, n)):
        assert L.dvae_swap_f32(*args, st) == EINVAL, args
    got, state = c.read()
    assert same_bits(got, draws[n]["e"]) and same_bits(state, np.array([0.9, 2, 0.25, 1, 1, *RESERVED], np.float32))


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_the_bits_and_twice_restores(draws, n):
    a0, b0 = draws[n]["e"].copy(), draws[n]["far"].copy()
    a0[0], b0[0], a0[-1], b0[-1] = np.float32(np.nan), -0.0, np.float32(1e-40), np.float32(-np.inf)     # bits, not values
    a, b = Buf(data=a0, lead=32), Buf(data=b0, lead=32)

    def swap():
        assert _lib.lib().dvae_swap_f32(a.ptr, b.ptr, n, _lib.stream()) == 0
        guards(a, b)
        return a.np(), b.np()

    x, y = swap()
    assert same_bits(x, b0) and same_bits(y, a0)
    x, y = swap()
    assert same_bits(x, a0) and same_bits(y, b0)


# ------------------------------------------------------------------ FlatAdam with the average on
SHAPES = [("p0", (37, 5)), ("p1", (1001,)), ("p2", (4, 4)), ("p3", (5000,))]      # as tests/test_hip_adam.py: 6208 elements
STATE_KEYS = {"format", "t", "lr", "betas", "eps", "names", "exp_avg", "exp_avg_sq"}


def make_opt(shapes=SHAPES, ema=None, warmup=True, max_norm=None, store_first=()):
    ps = [(name, torch.nn.Parameter(torch.from_numpy(params(40 + i, int(np.prod(shape)))).view(shape).to(DEV)))
          for i, (name, shape) in enumerate(shapes)]
    opt = FlatAdam(ps, lr=LR)
    if store_first:
        opt.set_store_first(store_first)
    if max_norm is not None:
        opt.set_grad_clip(max_norm)
    if ema is not None:
        opt.set_ema(ema, warmup=warmup)
    return opt


def feed(opt, seed):
    """This step's gradients, from the mixture, written into p.grad."""
    for i, p in enumerate(opt.params):
        p.grad.copy_(torch.from_numpy(grad_mixture(1000 * seed + i, p.numel())).view(p.shape))
        if getattr(p, "_dvae_grad_store_first", False):
            p._dvae_sf_writes = 1                      # written once, as the backward pass of a step does


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warm-up"])
@pytest.mark.parametrize("store_first", [(), ("p1",)], ids=["fold", "store_first"])
def test_three_steps_leave_adam_alone_and_the_average_follows_float64(store_first, warmup):
    off, on = make_opt(store_first=store_first), make_opt(ema=0.9, warmup=warmup, store_first=store_first)
    assert dev_equal(on.ema, on.flat_p) and on.ema_stats() == {"updates": 0, "weight": 0.0, "decay": 0.0, "applied": 0}
    for step in (1, 2, 3):
        feed(off, step)
        feed(on, step)
        e_before = down(on.ema)
        off.step(0.5)
        on.step(0.5)
        st = on.ema_stats()
        w_ref = weight_at(0.9, step, warmup)
        assert st["updates"] == step and st["applied"] == 1 and st["decay"] == float(np.float32(0.9))
        assert abs(st["weight"] - w_ref) <= TICK_REL * w_ref
        b = update_bounds(e_before, down(on.flat_p), st["weight"])        # the kernel's own p (after Adam) and w
        r, i = worst_ratio(down(on.ema), b["ref"], b["tol"])
        print(f"step {step}: average, worst error / bound = {r:.3f} at [{i}]")
        assert r <= 1.0
    a, b = flat(off), flat(on)
    for k in "pmvg":
        assert same_bits(a[k], b[k]), k
    assert off.t == on.t == 3 and same_bits(down(off.dev_state), down(on.dev_state))
    assert not dev_equal(on.ema, on.flat_p)
    assert not down(on.ema)[on.n_used:].any()                             # the zero tail stays zero
    with pytest.raises(RuntimeError, match="never switched on"):
        off.ema_stats()
    assert set(off.state_dict()) == STATE_KEYS and set(on.state_dict()) == STATE_KEYS | {"ema"}


def test_step_skipped_by_the_non_finite_guard_leaves_the_average_alone():
    opt = make_opt(ema=0.9, max_norm=math.inf)
    feed(opt, 1)
    opt.step()
    assert opt.ema_stats()["updates"] == 1 and opt.ema_stats()["applied"] == 1
    keep, state = opt.ema.clone(), opt.ema_state.clone()
    feed(opt, 2)
    opt.flat_g[17] = float("inf")
    opt.step()
    st = opt.ema_stats()
    assert opt.grad_clip_stats()["skipped"] == 1 and opt.t == 1
    assert dev_equal(opt.ema, keep) and st["updates"] == 1 and st["applied"] == 0
    assert dev_equal(opt.ema_state[0:4], state[0:4])
    feed(opt, 3)
    opt.step()
    st = opt.ema_stats()
    assert st["updates"] == 2 and st["applied"] == 1 and opt.t == 2 and not dev_equal(opt.ema, keep)
    assert abs(st["weight"] - weight_at(0.9, 2, True)) <= TICK_REL


def test_off_keeps_the_buffer_reset_starts_over_and_partial_ranges_never_update():
    opt = make_opt(ema=0.5)
    address = (opt.ema.data_ptr(), opt.ema_state.data_ptr())
    feed(opt, 1)
    opt.step()
    keep = opt.ema.clone()
    opt.set_ema(None)                                                     # the updates stop, the average stays
    feed(opt, 2)
    opt.step()
    assert opt.t == 2 and dev_equal(opt.ema, keep) and opt.ema_stats()["updates"] == 1
    opt.set_ema(0.5)                                                      # on again: continues, same buffers
    feed(opt, 3)
    opt.step_range(0, 1024, 1.0, tick=True)                               # a partial range: Adam there, no average
    opt.step_range(1024, opt.numel, 1.0, tick=False)
    assert opt.t == 3 and dev_equal(opt.ema, keep) and opt.ema_stats()["updates"] == 1
    feed(opt, 4)
    opt.step()
    assert opt.ema_stats()["updates"] == 2 and not dev_equal(opt.ema, keep)
    opt.set_ema(0.5, reset=True)
    assert dev_equal(opt.ema, opt.flat_p) and opt.ema_stats()["updates"] == 0 and opt.ema_stats()["applied"] == 0
    assert (opt.ema.data_ptr(), opt.ema_state.data_ptr()) == address      # allocated once: a captured graph holds them


def test_decay_is_a_device_scalar_and_capture_needs_it_sent(monkeypatch):
    opt = make_opt(ema=0.5, warmup=False)
    feed(opt, 1)
    opt.step()
    assert opt.ema_stats()["weight"] == 0.5 and opt.ema_stats()["decay"] == 0.5
    opt.set_ema(0.75, warmup=False)
    feed(opt, 1)
    before, e_before = flat(opt), down(opt.ema)
    # what step_range sees inside torch.cuda.graph(): the host value cannot be copied there, it has to be on the device
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="sync_scalars"):
        opt.step()
    with pytest.raises(RuntimeError, match="capture"):
        opt.swap_ema()
    monkeypatch.undo()
    after = flat(opt)
    assert all(same_bits(before[k], after[k]) for k in "pmvg") and opt.t == 1 and same_bits(e_before, down(opt.ema))
    opt.sync_scalars()
    assert float(opt.ema_state[0]) == 0.75 and opt.ema_stats()["updates"] == 1      # k and w lie between: not touched
    opt.step()
    assert opt.ema_stats() == {"updates": 2, "weight": 0.25, "decay": 0.75, "applied": 1}


def test_sharded_optimizer_with_the_average_on_is_refused():
    from dvae_amd.ddp import GradReducer

    class Stub:
        mode, world_size, rank = "rs_ag", 2, 0

    opt = make_opt(ema=0.9)
    w = dvae_amd.model.variational_base_vae.VariationalBaseModelVAE(None, 64, 80, 1, 32, 1e-3, DEV, 500, 4)
    w.optimizer = opt
    with pytest.raises(ValueError, match="rs_ag"):
        w.attach_reducer(Stub())
    assert w.reducer is None and opt.fold_zero_grad
    red = GradReducer.__new__(GradReducer)
    red.mode, red.world_size = "rs_ag", 2
    feed(opt, 1)
    before, e_before = flat(opt), down(opt.ema)
    with pytest.raises(ValueError, match="rs_ag"):
        red.step(opt)
    after = flat(opt)
    assert all(same_bits(before[k], after[k]) for k in "pmvg") and opt.t == 0 and same_bits(e_before, down(opt.ema))
    opt.set_ema(None)
    w.attach_reducer(Stub())                                        # the average off: attached as before
    assert w.reducer is not None and not opt.fold_zero_grad


def test_swap_and_the_context_manager():
    opt = make_opt(ema=0.9)
    for step in (1, 2):
        feed(opt, step)
        opt.step()
    p0, e0 = opt.flat_p.clone(), opt.ema.clone()
    address = [p.data_ptr() for p in opt.params]
    opt.swap_ema()
    assert opt.ema_swapped and dev_equal(opt.flat_p, e0) and dev_equal(opt.ema, p0)
    assert [p.data_ptr() for p in opt.params] == address and opt.views_intact()      # every parameter is the view it was
    o = opt.offsets["p3"]
    assert dev_equal(opt.params[3].data.view(-1), e0[o:o + 5000])
    feed(opt, 3)
    before = flat(opt)
    with pytest.raises(RuntimeError, match="swapped"):
        opt.step()
    with pytest.raises(RuntimeError, match="swapped"):
        opt.set_ema(0.9, reset=True)
    assert all(same_bits(before[k], flat(opt)[k]) for k in "pmvg") and opt.t == 2
    avg = {n: v.clone() for n, v in opt.state_dict()["ema"]["avg"].items()}          # the average, whichever side it is on
    opt.swap_ema()
    assert not opt.ema_swapped and dev_equal(opt.flat_p, p0) and dev_equal(opt.ema, e0)
    assert all(torch.equal(v, avg[n]) for n, v in opt.state_dict()["ema"]["avg"].items())
    with opt.ema_weights():
        assert opt.ema_swapped and dev_equal(opt.flat_p, e0)
    assert not opt.ema_swapped and dev_equal(opt.flat_p, p0) and dev_equal(opt.ema, e0)
    with pytest.raises(KeyError, match="from the body"):
        with opt.ema_weights():
            raise KeyError("from the body")
    assert not opt.ema_swapped and dev_equal(opt.flat_p, p0) and dev_equal(opt.ema, e0)
    opt.step()                                                            # and training goes on
    assert opt.t == 3 and opt.ema_stats()["updates"] == 3


def test_state_dict_carries_the_average_and_load_restores_it():
    src = make_opt(ema=0.9)
    for step in (1, 2, 3):
        feed(src, step)
        src.step()
    sd = src.state_dict()
    assert set(sd) == STATE_KEYS | {"ema"} and set(sd["ema"]) == {"decay", "warmup", "updates", "avg"}
    assert sd["ema"]["decay"] == 0.9 and sd["ema"]["warmup"] is True and sd["ema"]["updates"] == 3 and sd["format"] == 2
    assert list(sd["ema"]["avg"]) == src.names and tuple(sd["ema"]["avg"]["p0"].shape) == (37, 5)
    dst = make_opt(ema=0.5, warmup=False)                                 # the decay stays the caller's, not the file's
    dst.flat_p.copy_(src.flat_p)
    dst.load_state_dict(sd)
    assert dev_equal(dst.ema, src.ema) and dst.ema_stats()["updates"] == 3 and dst.ema_decay == 0.5
    feed(dst, 4)
    dst.step()
    assert dst.ema_stats() == {"updates": 4, "weight": 0.5, "decay": 0.5, "applied": 1}        # continues from k
    plain = make_opt()
    plain.load_state_dict(sd)                                             # the average off: the key is ignored
    assert plain.ema is None and set(plain.state_dict()) == STATE_KEYS
    old = {k: v for k, v in sd.items() if k != "ema"}
    dst.load_state_dict(old)                                              # a file without one: start from the weights
    assert dev_equal(dst.ema, dst.flat_p) and dst.ema_stats()["updates"] == 0


# ------------------------------------------------------------------ the whole step
def eval_forward(w, x1, x2, eps):
    w.model.eval()
    w.model.eps_override = eps
    try:
        with torch.no_grad():
            return [t.clone() for t in w.model(x1, x2, train=False)]
    finally:
        w.model.train()


def test_replayed_graph_equals_eager_step_with_the_average_on(tmp_path):
    """config 0 at B = 4 / T = 64: five steps, graph against eager, bit for bit, the average included.  Then the decay changes
    under the SAME graph, switching the average off captures another, and a forward under ema_weights() is the forward of a
    model that loaded the averaged state dict."""
    from oracle.fill import synthetic_eps, synthetic_pair
    B, T = 4, 64
    a, b = make_trainer(B, T), make_trainer(B, T)
    b.enable_graph(True)
    data = [tuple(t.cuda() for t in synthetic_pair(B, T, 700 + i)) for i in range(3)]
    noise = [synthetic_eps(B, seed=800 + i) for i in range(3)]

    def both(i):
        x1, x2 = data[i % 3]
        a.model.eps_override = b.model.eps_override = noise[(2 * i) % 3]
        la, lb = a.step(x1, x2, None, train=True), b.step(x1, x2, None, train=True)
        assert la == lb, (i, la, lb)
        for name in ("flat_p", "exp_avg", "exp_avg_sq", "ema"):
            assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), (i, name)
        sa, sb = a.optimizer.ema_stats(), b.optimizer.ema_stats()
        assert sa == sb, (i, sa, sb)
        return sa

    for w in (a, b):
        w.optimizer.set_ema(0.9)
    for i in range(5):
        st = both(i)
        assert st["updates"] == i + 1 and st["applied"] == 1
    assert abs(st["weight"] - weight_at(0.9, 5, True)) <= TICK_REL and a.optimizer.t == b.optimizer.t == 5
    graph = b._graph
    assert graph is not None and ("ema",) in b._graph_sig
    for w in (a, b):
        w.optimizer.set_ema(0.25)
    st = both(5)
    assert b._graph is graph and st["weight"] == 0.75 and st["decay"] == 0.25 and st["updates"] == 6      # no re-capture

    # the averaged weights: swapped in, saved, loaded by a second model
    x1, x2 = data[0]
    plain = eval_forward(b, x1, x2, noise[0])
    path = str(tmp_path / "DisentangledVAE_VCTK_1.ema.pth")
    p_before = b.optimizer.flat_p.clone()
    with b.ema_weights():
        averaged = eval_forward(b, x1, x2, noise[0])
        torch.save(b.model.state_dict(), path)
    assert dev_equal(b.optimizer.flat_p, p_before)
    assert all(bool(torch.isfinite(t).all()) for t in averaged)
    assert not dev_equal(averaged[0], plain[0]), "the averaged weights give the plain forward"
    again = eval_forward(b, x1, x2, noise[0])
    assert all(dev_equal(x, y) for x, y in zip(again, plain))                   # and the weights are back
    c = make_trainer(B, T)
    c.model.load_state_dict(torch.load(path, map_location="cuda"))
    loaded = eval_forward(c, x1, x2, noise[0])
    assert all(dev_equal(x, y) for x, y in zip(loaded, averaged))
    del c

    for w in (a, b):
        w.optimizer.set_ema(None)
    keep = b.optimizer.ema.clone()
    a.model.eps_override = b.model.eps_override = noise[0]
    la, lb = a.step(*data[0], None, train=True), b.step(*data[0], None, train=True)
    assert la == lb and dev_equal(a.optimizer.flat_p, b.optimizer.flat_p)
    assert b._graph is not None and b._graph is not graph and ("ema",) not in b._graph_sig      # other launches: captured again
    assert dev_equal(b.optimizer.ema, keep) and a.optimizer.t == b.optimizer.t == 7


def test_stopped_and_resumed_run_ends_with_the_same_average(tmp_path):
    """run_training for two epochs in one go against one epoch, a checkpoint, and a NEW trainer that resumes for the second:
    weights, moments and the average end bit-identical.  The EAGER step on a fixed list of batches: the command line's data
    streams (shuffles, crops) are not part of a checkpoint, so two of its runs see different batches after a resume whatever
    the optimiser does, and graph-against-eager is the test above."""
    from oracle.fill import synthetic_pair
    B, T = 4, 64
    loader = [tuple(t.cuda() for t in synthetic_pair(B, T, 900 + i)) + (torch.zeros(B, dtype=torch.long),) for i in range(3)]

    def trainer():
        w = make_trainer(B, T)
        w.optimizer.set_ema(0.9)
        return w

    def run(w, ckpt, epochs, resume):
        return w.run_training(loader, None, epochs, 1, reload_model=resume, checkpoints_path=str(ckpt),
                              logging_func=lambda *_: None)

    torch.cuda.manual_seed(5)
    whole = trainer()
    hist = run(whole, tmp_path / "whole", 2, False)
    assert [h["EMA/Updates"] for h in hist] == [3, 6]
    torch.cuda.manual_seed(5)
    first = trainer()
    run(first, tmp_path / "parts", 1, False)
    assert sorted(os.listdir(tmp_path / "parts")) == ["DisentangledVAE_VCTK_1.ema.pth", "DisentangledVAE_VCTK_1.opt",
                                                      "DisentangledVAE_VCTK_1.pth"]
    del first
    torch.cuda.manual_seed(77)                                            # the checkpoint brings the generator back
    second = trainer()
    hist2 = run(second, tmp_path / "parts", 1, True)
    assert [h["epoch"] for h in hist2] == [2] and hist2[0]["EMA/Updates"] == 6
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "ema"):
        assert dev_equal(getattr(whole.optimizer, name), getattr(second.optimizer, name)), name
    assert hist2[0] == hist[1]
    a = torch.load(tmp_path / "whole" / "DisentangledVAE_VCTK_2.ema.pth")
    b = torch.load(tmp_path / "parts" / "DisentangledVAE_VCTK_2.ema.pth")
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------ the command line
LOSS_KEYS = {"epoch", "Loss/Reconstruction Loss1", "Loss/Reconstruction Loss2", "Loss/Reconstruction Loss1 hat",
             "Loss/Reconstruction Loss2 hat", "Loss/Z1 KL Loss", "Loss/Z2 KL Loss", "Loss/Z KL Style"}
EMA_KEYS = {"EMA/Updates", "EMA/Weight"}
BASE = "DisentangledVAE_VCTK_2"


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """Two training runs of the command line on one synthetic corpus, shared by the tests below: two epochs of four steps
    with --ema-decay 0.9 (which also voices one conversion with the last iterate), and the same without."""
    from dvae_amd.data import write_synthetic_corpus
    root = tmp_path_factory.mktemp("ema_cli")
    corpus = write_synthetic_corpus(str(root / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)      # 16 pairs
    common = [f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4", "--epochs=2",
              "--report-interval=2", "--mse_cof=10", "--kl_cof=10", "--seed=3", "--src_spk=spk000", "--trg_spk=spk001",
              "--convert-count=1", "--griffin-lim-iters=2"]
    out = {"corpus": corpus, "common": common}
    for name, extra in (("ema", ["--ema-decay", "0.9", "--convert", "true"]), ("plain", [])):
        log_dir = root / name
        child("train", ["--train", "true", "--do-not-resume", f"--log_dir={log_dir}"] + common + extra)
        out[name] = log_dir
    return out


def _records(log_dir):
    return [json.loads(line) for line in open(log_dir / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]


def test_train_cli_writes_the_averaged_checkpoint(cli_runs):
    ck = cli_runs["ema"] / "checkpoints"
    assert sorted(os.listdir(ck)) == [BASE + ".ema.pth", BASE + ".opt", BASE + ".pth"]
    assert json.load(open(cli_runs["ema"] / "config.json"))["ema_decay"] == 0.9
    recs = _records(cli_runs["ema"])
    assert [r["epoch"] for r in recs] == [1, 2]
    for r in recs:
        assert set(r) == LOSS_KEYS | EMA_KEYS, set(r) ^ (LOSS_KEYS | EMA_KEYS)
        assert all(math.isfinite(v) for v in r.values()), r
        k = 4 * r["epoch"]
        assert r["EMA/Updates"] == k and abs(r["EMA/Weight"] - weight_at(0.9, k, True)) <= TICK_REL, r
    sd, avg, osd = (torch.load(ck / (BASE + ext), map_location="cpu") for ext in (".pth", ".ema.pth", ".opt"))
    assert list(sd) == list(avg) and all(sd[k].shape == avg[k].shape and sd[k].dtype == avg[k].dtype for k in sd)
    names = set(osd["names"])
    differ = {k for k in sd if not torch.equal(sd[k], avg[k])}
    buffers = [k for k in sd if k not in names]
    assert buffers and any("running_mean" in k for k in buffers) and not differ & set(buffers)      # BatchNorm: not averaged
    assert "enc_linear.linear_layer.weight" in differ and len(differ) > len(names) // 2, sorted(differ)[:5]
    assert all(bool(torch.isfinite(avg[k]).all()) for k in avg)
    ema = osd["ema"]
    assert ema["decay"] == 0.9 and ema["warmup"] is True and ema["updates"] == 8 and osd["format"] == 2
    assert list(ema["avg"]) == list(osd["exp_avg"])
    assert all(torch.equal(ema["avg"][n], avg[n]) for n in names), "the .opt's average is not the .ema.pth's parameters"


def test_plain_run_is_what_it_was(cli_runs):
    assert sorted(os.listdir(cli_runs["plain"] / "checkpoints")) == [BASE + ".opt", BASE + ".pth"]
    recs = _records(cli_runs["plain"])
    assert [r["epoch"] for r in recs] == [1, 2] and all(set(r) == LOSS_KEYS for r in recs), recs
    osd = torch.load(cli_runs["plain"] / "checkpoints" / (BASE + ".opt"), map_location="cpu")
    assert set(osd) == STATE_KEYS | {"cuda_rng_state", "cuda_rng_seed", "cuda_rng_offset"}
    assert json.load(open(cli_runs["plain"] / "config.json"))["ema_decay"] == 0.0
    # the two runs saw the same batches and noise: the average rides along, it does not steer
    a = torch.load(cli_runs["plain"] / "checkpoints" / (BASE + ".pth"), map_location="cpu")
    b = torch.load(cli_runs["ema"] / "checkpoints" / (BASE + ".pth"), map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_convert_use_ema_voices_the_average(cli_runs):
    gen = cli_runs["ema"] / "generation" / "spk000_to_spk001"
    mel, wav = gen / "convert_spk000_to_spk001_utt000.npy", gen / "convert_spk000_to_spk001_utt000.wav"
    last = np.load(mel)
    assert wav.is_file() and np.isfinite(last).all()
    os.remove(wav)
    child("train", ["--convert", "true", "--use-ema", f"--log_dir={cli_runs['ema']}"] + cli_runs["common"])
    averaged = np.load(mel)
    assert wav.is_file() and wav.stat().st_size > 44
    assert averaged.shape == last.shape and np.isfinite(averaged).all() and not np.array_equal(averaged, last)
    r = child("train", ["--convert", "true", "--use-ema", f"--log_dir={cli_runs['plain']}"] + cli_runs["common"], ok=False)
    assert r.returncode != 0 and BASE + ".ema.pth" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not (cli_runs["plain"] / "generation" / "spk000_to_spk001" / "convert_spk000_to_spk001_utt000.npy").exists()


def test_probe_use_ema(cli_runs):
    out = cli_runs["ema"] / "probe_ema.json"
    args = [cli_runs["corpus"], "--log_dir", cli_runs["ema"], "--epochs", 2, "--seed", 1]
    child("probe", args + ["--use-ema", "--json", out])
    res = json.loads(out.read_text())
    assert res["use_ema"] is True and res["checkpoint_epoch"] == 2 and set(res["probes"]) == {"style", "content"}
    assert all(0.0 <= res["probes"][k]["held_out_accuracy"] <= 1.0 for k in res["probes"])
    r = child("probe", [cli_runs["corpus"], "--log_dir", cli_runs["plain"], "--epochs", 1, "--use-ema"], ok=False)
    assert r.returncode == 1 and BASE + ".ema.pth" in r.stderr, (r.returncode, r.stderr[-2000:])
