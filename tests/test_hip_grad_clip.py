"""Gradient-norm clipping and the non-finite step guard on the MI355X (csrc/elem.hip: grad_sumsq_kernel,
grad_clip_finalize_kernel, adam_tick_kernel<true>, adam_dev_kernel<U, true>; optim.FlatAdam.set_grad_clip) against the
float64 reference of tests/grad_clip_ref.py and tests/adam_ref.py.

The bounds are the ones derived in tests/grad_clip_ref.py: |norm - ref| <= 2^-23 ref, eff within 4 * 2^-24 of
gs max_norm / (ref_norm + 1e-6), eff == gs BIT FOR BIT where the coefficient clamps to 1; a clipped Adam step is held to
adam_ref's one-step bounds against the float64 Adam fed the kernel's OWN float32 eff, so the two checks compose and neither
hides the other.  Sizes reach every path of the reduction: one float4, either side of one workgroup trip (256 threads x 2
float4), and a few float4 past one full sweep of the capped grid (2048 workgroups), where the grid-stride loop makes a
second, ragged trip.  The workspace and clip_state lie in guarded buffers (tests/kernel_harness.py)."""
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import bits, Buf, DEV, child, dev_equal, down, flat, EINVAL, guards, make_trainer, same_bits
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib  # noqa: E402
from dvae_amd.optim import FlatAdam  # noqa: E402
from adam_ref import BETAS, EPS, LR, bias_corrections, grad_mixture, one_step_bounds, params, worst_ratio  # noqa: E402
from grad_clip_ref import clip_ref, eff_tol, norm_tol, sum_squares  # noqa: E402

U, CAP = 2, 2048                              # SUMSQ_U, SUMSQ_CAP of csrc/elem.hip
TRIP = 4 * 256 * U                            # elements one workgroup reads per trip
SWEEP = CAP * TRIP                            # ... and the whole capped grid: 4 194 304
SIZES = [4, TRIP - 4, TRIP, TRIP + 4, SWEEP + 4 * 259]      # the last: 256 threads with a first float4, 3 with a second
SENT = -7.5e11
B1F, B2F, EPSF, LRF = (np.float32(x) for x in (BETAS[0], BETAS[1], EPS, LR))


# ------------------------------------------------------------------ the two new launches through ctypes
class Clip:
    """g, the float64 workspace and clip_state on the device, the latter two in guarded buffers, 64 and 32 bytes behind a
    multiple of 256; the workspace starts as the sentinel."""

    def __init__(self, g, gs, max_norm):
        L = _lib.lib()
        self.n = int(g.size)
        self.g = torch.tensor(np.asarray(g, np.float32), device=DEV)
        self.g0 = self.g.clone()
        self.nws = int(L.dvae_grad_sumsq_ws_bytes(self.n)) // 8
        assert self.nws == min(CAP, max(1, -(-(self.n // 4) // (256 * U)))), (self.n, self.nws)
        self.ws = Buf(data=np.full(self.nws, SENT, np.float64), lead=64)
        self.clip = Buf(data=np.array([max_norm, 0, 0, 0, 0, 0, 0, 0], np.float32), lead=32)
        self.state = torch.tensor([3, 0.271, 0.0547, SENT, float(LRF), gs, SENT, SENT], dtype=torch.float32, device=DEV)
        self.state0 = self.state.clone()

    def run(self, guard=1, skip=None):
        L = _lib.lib()
        assert L.dvae_grad_sumsq(self.g.data_ptr(), self.n, self.ws.ptr, _lib.stream()) == 0
        assert L.dvae_grad_clip_finalize(self.ws.ptr, self.n, self.state.data_ptr(), self.clip.ptr,
                                         None if skip is None else skip.data_ptr(), guard, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert dev_equal(self.g, self.g0) and dev_equal(self.state, self.state0)          # read-only inputs
        guards(self.ws, self.clip)
        return self.clip.np(), self.ws.np()


@pytest.fixture(scope="module")
def draws():
    """One gradient draw per size and its exactly rounded sum of squares, shared by the tests below and left unchanged."""
    out = {}
    for n in SIZES:
        g = grad_mixture(n % 997, n)
        g.setflags(write=False)
        out[n] = (g, sum_squares(g))
    return out


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_float64_and_bit_identical_twice(draws, n, gs):
    g, s = draws[n]
    ref_norm = clip_ref(g, gs, math.inf, sumsq=s)[0]
    c = Clip(g, gs, math.inf)
    first, part1 = c.run()
    second, part2 = c.run()
    err = abs(float(first[1]) - ref_norm)
    print(f"n={n} gs={gs}: norm {first[1]!r}, reference {ref_norm!r}, error / bound = {err / norm_tol(ref_norm):.3f}")
    assert err <= norm_tol(ref_norm)
    assert np.array_equal(part1.view(np.uint64), part2.view(np.uint64)) and same_bits(first, second)
    assert abs(math.fsum(part1.tolist()) - s) <= n * 2.0 ** -53 * s          # the partials themselves add up to the sum
    assert first[2] == 1.0 and same_bits(first[3], np.float32(gs))           # inf never clips
    assert first[4] == 0 and first[5] == 0 and first[6] == 0 and first[7] == 0
    assert first[0] == np.float32(np.inf)                                    # max_norm is the host's: not written


@pytest.mark.parametrize("n", [4, TRIP + 4])
def test_all_zero_gradient(n):
    out, _ = Clip(np.zeros(n, np.float32), 0.5, 1.0).run()
    assert out[1] == 0.0 and out[2] == 1.0 and same_bits(out[3], np.float32(0.5)) and not out[4:].any()


@pytest.mark.parametrize("gs", [1.0, 0.5, float(np.float32(1.0 / 3.0))])
def test_clamp_is_exact(draws, gs):
    """max_norm = inf and max_norm = twice the measured norm: eff is grad_scale, bit for bit."""
    g, _ = draws[TRIP + 4]
    measured = Clip(g, gs, math.inf).run()[0][1]
    for max_norm in (math.inf, 2.0 * float(measured)):
        out, _ = Clip(g, gs, max_norm).run()
        assert out[2] == 1.0 and same_bits(out[3], np.float32(gs)) and out[6] == 0, (max_norm, out)


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("n", SIZES)
def test_clipped_coefficient_against_float64(draws, n, gs):
    g, s = draws[n]
    max_norm = np.float32(0.1 * clip_ref(g, gs, math.inf, sumsq=s)[0])
    norm, coef, eff, _ = clip_ref(g, gs, max_norm, sumsq=s)
    c = Clip(g, gs, max_norm)
    out, _ = c.run()
    print(f"n={n} gs={gs}: eff {out[3]!r}, reference {eff!r}, error / bound = {abs(float(out[3]) - eff) / eff_tol(eff):.3f}")
    assert abs(float(out[3]) - eff) <= eff_tol(eff)
    assert abs(float(out[2]) - coef) <= eff_tol(coef) and abs(float(out[1]) - norm) <= norm_tol(norm)
    assert out[4] == 0 and out[5] == 0 and out[6] == 1 and out[7] == 0
    assert c.run()[0][6] == 2                                                # the counter counts


def test_finalize_honours_the_skip_word_and_refuses_bad_arguments(draws):
    g, _ = draws[TRIP + 4]
    c = Clip(g, 1.0, 1.0)
    word = torch.tensor([2, 0, 0, 0], dtype=torch.uint8, device=DEV)          # a uint32 holding 2
    out, _ = c.run(skip=word)
    assert same_bits(out, np.array([1, 0, 0, 0, 0, 0, 0, 0], np.float32))     # nothing, counters included
    word.zero_()
    out, _ = c.run(skip=word)
    assert out[1] > 0 and out[6] == 1
    L, st = _lib.lib(), _lib.stream()
    ws, clip, state = c.ws.ptr, c.clip.ptr, c.state.data_ptr()
    before = c.clip.np()
    assert L.dvae_grad_sumsq_ws_bytes(0) == 0 and L.dvae_grad_sumsq_ws_bytes(6) == 0
    for args in ((None, c.n, ws, st), (c.g.data_ptr(), 0, ws, st), (c.g.data_ptr(), 6, ws, st), (c.g.data_ptr(), c.n, None, st),
                 (c.g.data_ptr() + 4, c.n - 4, ws, st), (c.g.data_ptr(), c.n, ws + 4, st)):
        assert L.dvae_grad_sumsq(*args) == EINVAL, args
    for args in ((None, c.n, state, clip), (ws, 2, state, clip), (ws, c.n, None, clip), (ws, c.n, state, None)):
        assert L.dvae_grad_clip_finalize(*args, None, 1, st) == EINVAL, args
    a = [c.g.data_ptr()] * 4
    assert L.dvae_adam_flat_dev_clip(*a, c.n, 0.9, 0.999, 1e-8, state, None, None, 1, None, st) == EINVAL
    guards(c.ws, c.clip)
    assert same_bits(before, c.clip.np())


# ------------------------------------------------------------------ FlatAdam with clipping on
SHAPES = [("p0", (37, 5)), ("p1", (1001,)), ("p2", (4, 4)), ("p3", (5000,))]      # as tests/test_hip_adam.py: 6208 elements


def make_opt(shapes=SHAPES, max_norm=None, skip_nonfinite=True, store_first=()):
    ps = [(name, torch.nn.Parameter(torch.from_numpy(params(40 + i, int(np.prod(shape)))).view(shape).to(DEV)))
          for i, (name, shape) in enumerate(shapes)]
    opt = FlatAdam(ps, lr=LR)
    if store_first:
        opt.set_store_first(store_first)
    if max_norm is not None:
        opt.set_grad_clip(max_norm, skip_nonfinite=skip_nonfinite)
    return opt


def feed(opt, seed, scale=1.0):
    """This step's gradients, from the mixture, written into p.grad; the whole flat gradient comes back (float32)."""
    for i, p in enumerate(opt.params):
        g = grad_mixture(1000 * seed + i, p.numel()) * np.float32(scale)
        p.grad.copy_(torch.from_numpy(g).view(p.shape))
        if getattr(p, "_dvae_grad_store_first", False):
            p._dvae_sf_writes = 1                      # written once, as the backward pass of a step does
    return down(opt.flat_g)


def zero_mask(opt):
    mask = np.zeros(opt.numel, dtype=bool)
    for a, b in opt._zero_ranges:
        mask[a:b] = True
    return mask


def check_against_float64(before, after, state, eff, cleared, what, p_tol="tol_p"):
    """`after` is one Adam step from `before` with the scalars the device holds and `eff` as the gradient scale.  p_tol:
    "tol_p_cancel" where the gradient may have changed sign against the first moment (tests/adam_ref.py)."""
    sc = (state[4], B1F, B2F, EPSF, np.float32(eff), state[1], state[2])
    b = one_step_bounds(before["p"], before["g"], before["m"], before["v"], *sc, cancel=(p_tol != "tol_p"))
    for k in "mvp":
        r, i = worst_ratio(after[k], b["ref_" + k], b[p_tol if k == "p" else "tol_" + k])
        assert r <= 1.0, (f"{what}: {k}[{i}] = {after[k][i]!r}, reference {b['ref_' + k][i]!r}, error / bound = {r:.3f}")
    assert not bits(after["g"][cleared]).any(), f"{what}: a gradient inside a clear range is not +0.0"
    assert same_bits(before["g"][~cleared], after["g"][~cleared]), f"{what}: a gradient outside the clear ranges changed"


def check_tick(state, t):
    assert state[0] == np.float32(t), (state[0], t)
    bc1, bc2s = bias_corrections(float(B1F), float(B2F), t)
    assert abs(float(state[1]) - bc1) <= 2.0 ** -23 * bc1 and abs(float(state[2]) - bc2s) <= 2.0 ** -23 * bc2s


@pytest.mark.parametrize("store_first", [(), ("p1",)], ids=["fold", "store_first"])
def test_unclipped_steps_are_bit_identical_to_clipping_off(store_first):
    """max_norm = inf, and max_norm = twice the largest norm of the three steps: p, m, v, g and t after three steps are those of
    FlatAdam with clipping off on the same gradients, and the statistics see every step."""
    norms = []
    for step in (1, 2, 3):
        probe = make_opt()
        norms.append(clip_ref(feed(probe, step), 0.5, math.inf)[0])
    for max_norm in (math.inf, 2.0 * max(norms)):
        off, on = make_opt(store_first=store_first), make_opt(max_norm=max_norm, store_first=store_first)
        for step in (1, 2, 3):
            feed(off, step)
            feed(on, step)
            off.step(0.5)
            on.step(0.5)
            st = on.grad_clip_stats()
            assert abs(st["norm"] - norms[step - 1]) <= norm_tol(norms[step - 1]) and st["coef"] == 1.0
            assert same_bits(down(on.clip_state)[3], np.float32(0.5))
        a, b = flat(off), flat(on)
        for k in "pmvg":
            assert same_bits(a[k], b[k]), (max_norm, k)
        assert off.t == on.t == 3 and same_bits(down(off.dev_state), down(on.dev_state))
        assert st["nonfinite"] == 0 and st["skipped"] == 0 and st["clipped"] == 0
    with pytest.raises(RuntimeError, match="never switched on"):
        off.grad_clip_stats()


@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_clipped_step_against_float64(gs):
    opt = make_opt(store_first=("p1",))
    g = feed(opt, 1)
    ref_norm = clip_ref(g, gs, math.inf)[0]
    max_norm = float(np.float32(0.1 * ref_norm))
    opt.set_grad_clip(max_norm)
    for step in (1, 2):                                # the same gradient twice: the second step has moments that are not zero
        feed(opt, 1)
        before = flat(opt)
        opt.step(gs)
        after, state, clip = flat(opt), down(opt.dev_state), down(opt.clip_state)
        norm, coef, eff, _ = clip_ref(before["g"], gs, max_norm)
        assert abs(float(clip[3]) - eff) <= eff_tol(eff), (clip[3], eff)
        assert 0.09 < clip[2] < 0.11 and clip[0] == np.float32(max_norm)
        check_tick(state, step)
        check_against_float64(before, after, state, clip[3], zero_mask(opt), f"gs={gs} step {step}")
        st = opt.grad_clip_stats()
        assert st["clipped"] == step and st["skipped"] == 0 and st["nonfinite"] == 0
        assert abs(st["norm"] - norm) <= norm_tol(norm)
    # the scale Adam used is eff, not grad_scale: the first moment of a plain step would be ten times this one
    assert np.abs(after["m"]).max() < 0.5 * np.abs(gs * before["g"]).max() * (1 - 0.9 ** 2)


def test_huge_but_finite_gradient_is_clipped_not_skipped():
    opt = make_opt(shapes=[("w", (4,))], max_norm=1.0)
    assert opt.numel == 32
    opt.params[0].grad.copy_(torch.tensor([3e38, -3e38, 3e38, -3e38]))
    before = flat(opt)
    opt.step()
    after, state, clip = flat(opt), down(opt.dev_state), down(opt.clip_state)
    st = opt.grad_clip_stats()
    assert st["norm"] == math.inf and st["nonfinite"] == 0 and st["skipped"] == 0 and st["clipped"] == 1
    norm, coef, eff, nonfinite = clip_ref(before["g"], 1.0, 1.0)
    assert not nonfinite and abs(float(clip[3]) - eff) <= eff_tol(eff), (clip[3], eff)
    check_tick(state, 1)
    check_against_float64(before, after, state, clip[3], zero_mask(opt), "huge")
    scaled = float(clip[3]) * before["g"][:4].astype(np.float64)
    assert np.allclose(scaled, [0.5, -0.5, 0.5, -0.5], rtol=1e-5), scaled
    # one step from zero moments with gradients of +-0.5: p moves by lr against the gradient's sign
    assert np.allclose(after["p"][:4] - before["p"][:4], [-LR, LR, -LR, LR], rtol=1e-3)


BIG = [("a", (1000,)), ("big", (SWEEP + 1000,)), ("c", (501,))]          # the flat buffer reaches into the second trip


@pytest.fixture(scope="module")
def big_opt():
    """One optimizer for every non-finite case: a skipped step leaves it where it was, which is what is being checked."""
    opt = make_opt(shapes=BIG, max_norm=math.inf, store_first=("a",))
    feed(opt, 1)
    opt.step()                                          # moments that are not zero
    assert opt.t == 1 and opt.n_used == 2000 + SWEEP + 504 and opt._zero_ranges == [(1000, opt.numel)]
    return opt


@pytest.mark.parametrize("where", ["first", "last", "second_trip"])
@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "+inf", "-inf"])
def test_non_finite_gradient_skips_the_step(big_opt, bad, where):
    opt = big_opt
    idx = {"first": 0, "last": opt.offsets["c"] + 500, "second_trip": SWEEP + 8}[where]      # last: in front of the zero tail
    t0, skipped0 = opt.t, opt.grad_clip_stats()["skipped"]
    feed(opt, 2)
    opt.flat_g[idx] = bad
    keep = {k: getattr(opt, k).clone() for k in ("flat_p", "exp_avg", "exp_avg_sq", "dev_state")}
    g_before = opt.flat_g.clone()
    opt.step()
    torch.cuda.synchronize()
    for k in ("flat_p", "exp_avg", "exp_avg_sq"):
        assert dev_equal(getattr(opt, k), keep[k]), (k, "changed by a skipped step")
    assert dev_equal(opt.dev_state[0:3], keep["dev_state"][0:3]) and opt.t == t0
    assert not opt.flat_g[1000:].view(torch.int32).any(), "the clear ranges of g are not zero after a skipped step"
    assert dev_equal(opt.flat_g[:1000], g_before[:1000])                     # store-first: outside the clear ranges
    st = opt.grad_clip_stats()
    assert st["nonfinite"] == 1 and st["skipped"] == skipped0 + 1 and st["clipped"] == 0 and not math.isfinite(st["norm"])
    assert opt._clean                                                        # the next zero_grad is still free
    # the following finite step is step t0 + 1, and a float64 Adam step from the untouched buffers
    feed(opt, 3)
    before = flat(opt)
    opt.step()
    after, state = flat(opt), down(opt.dev_state)
    check_tick(state, t0 + 1)
    assert opt.t == t0 + 1
    check_against_float64(before, after, state, 1.0, zero_mask(opt), f"after {bad} at {where}", p_tol="tol_p_cancel")
    st = opt.grad_clip_stats()
    assert st["nonfinite"] == 0 and st["skipped"] == skipped0 + 1 and math.isfinite(st["norm"])


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf], ids=["nan", "+inf", "-inf"])
def test_without_the_guard_the_same_gradient_updates(bad):
    opt = make_opt(max_norm=math.inf, skip_nonfinite=False)
    feed(opt, 1)
    opt.step()
    feed(opt, 2)
    opt.flat_g[0] = bad
    before = flat(opt)
    opt.step()
    after = flat(opt)
    st = opt.grad_clip_stats()
    assert opt.t == 2 and st["nonfinite"] == 1 and st["skipped"] == 0
    assert not np.isfinite(after["p"][0]) and not same_bits(before["p"][1:], after["p"][1:])


def test_max_norm_is_a_device_scalar_and_capture_needs_it_sent(monkeypatch):
    opt = make_opt(max_norm=5.0)
    feed(opt, 1)
    opt.step()
    assert float(opt.clip_state[0]) == 5.0 and opt.grad_clip_stats()["clipped"] == 1
    opt.set_grad_clip(7.0)
    feed(opt, 1)
    before = flat(opt)
    # what step_range sees inside torch.cuda.graph(): the host value cannot be copied there, it has to be on the device
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="sync_scalars"):
        opt.step()
    monkeypatch.undo()
    after = flat(opt)
    assert all(same_bits(before[k], after[k]) for k in "pmvg") and opt.t == 1          # refused before any launch
    opt.sync_scalars()
    assert float(opt.clip_state[0]) == 7.0
    opt.step()
    assert opt.t == 2 and opt.grad_clip_stats()["clipped"] == 2
    with pytest.raises(ValueError):
        opt.set_grad_clip(0.0)
    with pytest.raises(ValueError):
        opt.set_grad_clip(float("nan"))


# ------------------------------------------------------------------ the whole step
def test_replayed_graph_equals_eager_step_with_clipping_on():
    """config 0 at B = 4 / T = 64: the first step measures (max_norm = inf), then max_norm = 5 % of that norm so that every
    step clips; four steps, graph against eager, bit for bit.  Then max_norm changes under the SAME graph, and switching
    clipping off captures another."""
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
        for name in ("flat_p", "exp_avg", "exp_avg_sq"):
            assert dev_equal(getattr(a.optimizer, name), getattr(b.optimizer, name)), (i, name)
        sa, sb = a.optimizer.grad_clip_stats() if a.optimizer.max_norm is not None else None, None
        if sa is not None:
            sb = b.optimizer.grad_clip_stats()
            assert sa == sb, (i, sa, sb)
        return sa

    for w in (a, b):
        w.optimizer.set_grad_clip(math.inf)
    n0 = both(0)["norm"]
    assert math.isfinite(n0) and n0 > 0
    for w in (a, b):
        w.optimizer.set_grad_clip(0.05 * n0)
    coefs = [both(i)["coef"] for i in range(1, 5)]
    assert all(c < 1.0 for c in coefs), coefs
    assert a.optimizer.grad_clip_stats()["clipped"] == 4 and a.optimizer.t == b.optimizer.t == 5
    graph = b._graph
    assert graph is not None
    for w in (a, b):
        w.optimizer.set_grad_clip(0.005 * n0)
    st = both(5)
    assert b._graph is graph and st["coef"] < 0.3 * max(coefs) and st["clipped"] == 5      # took effect, no re-capture
    for w in (a, b):
        w.optimizer.set_grad_clip(None)
    both(6)
    assert b._graph is not None and b._graph is not graph                                   # other launches: captured again
    assert a.optimizer.t == b.optimizer.t == 7


def test_poked_inf_between_backward_and_step_leaves_the_parameters_finite():
    """An inf written into flat_g after the eager backward pass and before optimizer.step(): with the guard the step does
    not happen and every parameter stays finite; the same poke with clipping off puts a NaN into the weights."""
    from oracle.fill import synthetic_eps, synthetic_pair
    B, T = 4, 64
    w = make_trainer(B, T)
    opt = w.optimizer
    x1, x2 = (t.cuda() for t in synthetic_pair(B, T, 11))
    w.model.eps_override = synthetic_eps(B, seed=12)
    plain_step = opt.step

    def poked_step(grad_scale=1.0):
        opt.flat_g[5] = float("inf")
        return plain_step(grad_scale=grad_scale)

    opt.set_grad_clip(1e9)
    w.step(x1, x2, None, train=True)
    p0 = opt.flat_p.clone()
    opt.step = poked_step
    w.step(x1, x2, None, train=True)
    st = opt.grad_clip_stats()
    assert bool(torch.isfinite(opt.flat_p).all()) and dev_equal(opt.flat_p, p0) and opt.t == 1
    assert st["nonfinite"] == 1 and st["skipped"] == 1
    opt.step = plain_step
    losses = w.step(x1, x2, None, train=True)                       # training goes on
    assert opt.t == 2 and all(math.isfinite(v) for v in losses) and bool(torch.isfinite(opt.flat_p).all())
    opt.set_grad_clip(None)
    opt.step = poked_step
    w.step(x1, x2, None, train=True)
    assert not bool(torch.isfinite(opt.flat_p).all())               # what the guard is for


def test_sharded_optimizer_with_clipping_on_is_refused():
    from dvae_amd.ddp import GradReducer

    class Stub:
        mode, world_size, rank = "rs_ag", 2, 0

    opt = make_opt(max_norm=1.0)
    w = dvae_amd.model.variational_base_vae.VariationalBaseModelVAE(None, 64, 80, 1, 32, 1e-3, DEV, 500, 4)
    w.optimizer = opt
    with pytest.raises(ValueError, match="rs_ag"):
        w.attach_reducer(Stub())
    assert w.reducer is None and opt.fold_zero_grad
    red = GradReducer.__new__(GradReducer)
    red.mode, red.world_size = "rs_ag", 2
    feed(opt, 1)
    before = flat(opt)
    with pytest.raises(ValueError, match="rs_ag"):
        red.step(opt)
    after = flat(opt)
    assert all(same_bits(before[k], after[k]) for k in "pmvg") and opt.t == 0
    opt.set_grad_clip(None)
    w.attach_reducer(Stub())                                        # clipping off: attached as before
    assert w.reducer is not None and not opt.fold_zero_grad


# ------------------------------------------------------------------ the command line
LOSS_KEYS = {"epoch", "Loss/Reconstruction Loss1", "Loss/Reconstruction Loss2", "Loss/Reconstruction Loss1 hat",
             "Loss/Reconstruction Loss2 hat", "Loss/Z1 KL Loss", "Loss/Z2 KL Loss", "Loss/Z KL Style"}
GRAD_KEYS = {"Grad/Norm mean", "Grad/Norm max", "Grad/Clipped steps", "Grad/Skipped steps"}


def _cli(tmp_path, name, extra):
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=2, n_utt=16, length=96, seed=0)   # 16 pairs
    log_dir = tmp_path / name
    child("train", ["--train", "true", f"--dataset_fp={corpus}", "--batch-size=4", "--latent-size=32", "--speaker_size=4", "--lr=1e-4",
                    "--epochs=2", "--report-interval=2", "--mse_cof=10", "--kl_cof=10", f"--log_dir={log_dir}", "--seed=3",
                    "--do-not-resume"] + extra)
    recs = [json.loads(line) for line in open(log_dir / "logs" / "DisentangledVAE_VCTK" / "scalars.jsonl")]
    return recs, json.load(open(log_dir / "config.json"))


def test_train_cli_clip_grad_norm_logs_the_norm(tmp_path):
    recs, config = _cli(tmp_path, "clipped", ["--clip-grad-norm", "0.5"])
    assert config["clip_grad_norm"] == 0.5 and config["log_grad_norm"] is False
    assert [r["epoch"] for r in recs] == [1, 2]
    for r in recs:
        assert set(r) == LOSS_KEYS | GRAD_KEYS, set(r) ^ (LOSS_KEYS | GRAD_KEYS)
        assert all(math.isfinite(v) for v in r.values()), r
        assert r["Grad/Norm max"] >= r["Grad/Norm mean"] > 0, r
        assert r["Grad/Skipped steps"] == 0 and 0 <= r["Grad/Clipped steps"] <= 4, r
    recs, config = _cli(tmp_path, "plain", [])
    assert config["clip_grad_norm"] == 0.0
    assert [r["epoch"] for r in recs] == [1, 2] and all(set(r) == LOSS_KEYS for r in recs), recs
