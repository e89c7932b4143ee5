"""The Adam step kernels on the MI355X (csrc/elem.hip: adam_tick_kernel, adam_dev_kernel, adam_kernel) against the float64
reference of tests/adam_ref.py, element by element.

Every kernel comparison is ONE step from the device's own buffers: p, g, m, v and dev_state are downloaded before the
launch, `adam_step_ref` runs in float64 on those float32 values with the float32 scalars the device holds, and the result
is compared with what the launch left.  No error accumulates, so the bounds are the rounding bounds derived in
tests/adam_ref.py (eps32 = 2^-24, floor 2^-126):
    |m' - ref| <= 4 eps32 (|m| + |gs g|)      |v' - ref| <= 4 eps32 ref      |p' - ref| <= eps32 |ref| + 12 eps32 |u|
Each buffer is a guarded one of tests/kernel_harness.py: the 256 bytes on either side must keep their bits.
Inputs: p uniform in +-1, g drawn from {0, +-1e-30, +-1e-12, +-1e-8, +-1e-4, +-1, +-1e3} (sqrt(v) far below, near and far
above eps), m = v = 0 before the first step and whatever the previous step left afterwards.

The p bound counts the first moment as four roundings relative to ITSELF, which holds while m and gs*g do not cancel: in
every raw-kernel test here (the same gradient launch after launch) and in the sharded / checkpoint tests.  In the 20-step
FlatAdam run the gradient changes sign between steps and m' = 0.9 m + 0.1 g can cancel; tests/adam_ref.py derives
the form that carries the absolute error of m' through the division (`tol_p_cancel`) and shows on an fp32 restatement that
the two differ only for an element with |p| < 1e-3 whose first moment cancelled.  The 20-step run is held to both: the
12-rounding bound as stated has a test of its own (test_flat_adam_twenty_steps_p_meets_the_twelve_rounding_bound).
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import bits, Buf, DEV, down, EINVAL, flat, guards, same_bits, st, sync, Worst      # first: it puts the repository root on sys.path
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib  # noqa: E402
from dvae_amd._lib import Ranges  # noqa: E402
from dvae_amd.optim import FlatAdam  # noqa: E402
from adam_ref import BETAS, EPS, EPS32, LR, bias_corrections, grad_mixture, one_step_bounds, params, worst_ratio  # noqa: E402

SENT = np.float32(-7.5e11)                 # no step produces it
B1F, B2F, EPSF, LRF = (np.float32(x) for x in (BETAS[0], BETAS[1], EPS, LR))
BLOCK = 2048                               # elements per block and trip: 256 threads x 2 float4
SIZES = [4, 1020, 1024, 1028, 2052, 4 * (2 * 1048576 + 256 + 3)]
WORST = Worst("test_hip_adam.py")          # over every raw-kernel and FlatAdam comparison of this module (printed at the end)
WORST.worst.update(m=0.0, v=0.0, p=0.0)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def arena(n, seed):
    """p, g, m, v of n floats, each in a guarded buffer of its own."""
    return {k: Buf(data=a) for k, a in (("p", params(seed, n)), ("g", grad_mixture(seed + 1, n)), ("m", np.zeros(n, np.float32)),
                                        ("v", np.zeros(n, np.float32)))}


def snap(ar):
    """p, g, m, v as they are now; no launch so far wrote outside them."""
    guards(*ar.values())
    return {k: ar[k].np() for k in "pgmv"}


def new_state(lr=LRF, gs=1.0):
    """dev_state with the unused words set to the sentinel: [t, 1-b1^t, sqrt(1-b2^t), -, lr, grad_scale, -, -]."""
    s = np.array([0, 0, 0, SENT, lr, gs, SENT, SENT], dtype=np.float32)
    return torch.from_numpy(s).to(DEV)


def ranges(spans, n=None):
    rg = Ranges()
    rg.n = len(spans) if n is None else n
    for i, (a, b) in enumerate(spans):
        rg.lo[i], rg.hi[i] = a, b
    return rg


def launch_dev(ar, state, n=None, skip=None, clear=None, tick=1, offsets=(0, 0, 0, 0)):
    rc = _lib.lib().dvae_adam_flat_dev(*(ar[k].ptr + o for k, o in zip("pgmv", offsets)), ar["p"].shape[0] if n is None else n,
                                       float(B1F), float(B2F), float(EPSF), state.data_ptr(),
                                       None if skip is None else skip.data_ptr(),
                                       None if clear is None else C.byref(clear), tick, st())
    sync()
    return rc


def unchanged(before, after, what=""):
    for k in before:
        assert same_bits(before[k], after[k]), f"{what}: {k} changed"


def check_step(before, after, sc, cleared=None, p_tol="tol_p", what=""):
    """`after` is one step from `before` (`snap`, which has checked the guards, or whole flat buffers) with the scalars
    sc = (lr, b1, b2, eps, gs, bc1, bc2s); g is zero where `cleared` (a mask over [0, n)) and untouched elsewhere."""
    n = len(before["p"])
    g0, g1 = before["g"], after["g"]
    if cleared is None:
        cleared = np.zeros(n, dtype=bool)
    assert not bits(g1[cleared]).any(), f"{what}: a gradient inside a clear range is not +0.0"
    assert same_bits(g0[~cleared], g1[~cleared]), f"{what}: a gradient outside the clear ranges changed"
    b = one_step_bounds(before["p"], g0, before["m"], before["v"], *sc, cancel=(p_tol != "tol_p"))
    out = {}
    for k, tol in (("m", "tol_m"), ("v", "tol_v"), ("p", p_tol)):
        r, i = worst_ratio(after[k], b["ref_" + k], b[tol])
        out[k] = r
        if p_tol == "tol_p" or k != "p":
            WORST.record(k, r)
        assert r <= 1.0, (f"{what}: {k}[{i}] = {after[k][i]!r}, reference {b['ref_' + k][i]!r}, error / bound = {r:.3f} "
                          f"(before: p {before['p'][i]!r} g {g0[i]!r} m {before['m'][i]!r} v {before['v'][i]!r})")
    return out


def ulps(a, b):
    return abs(int(bits(np.float32(a)).item()) - int(bits(np.float32(b)).item()))


def check_tick(s0, s1, t):
    """dev_state after the tick to step t: the counter, both bias corrections within 1 ulp of their double value from the
    float32 betas; the unused words, lr and grad_scale keep their bits."""
    assert s1[0] == np.float32(t), (s1[0], t)
    bc1, bc2s = bias_corrections(float(B1F), float(B2F), t)
    assert ulps(s1[1], bc1) <= 1, (t, s1[1], bc1)
    assert ulps(s1[2], bc2s) <= 1, (t, s1[2], bc2s)
    assert same_bits(s0[3:], s1[3:]), (s0, s1)


def scalars(state_np):
    return (state_np[4], B1F, B2F, EPSF, state_np[5], state_np[1], state_np[2])


# ------------------------------------------------------------------ dvae_adam_flat_dev through ctypes
@pytest.mark.parametrize("n", SIZES)
def test_dev_five_ticking_launches(n):
    """Sizes where only some threads have a second float4 (the clamped load, the guarded store), one block plus one float4,
    and two full grid-stride sweeps plus a ragged third."""
    ar, state = arena(n, seed=n % 1000), new_state()
    for t in range(1, 6):
        before, s0 = snap(ar), down(state)
        assert launch_dev(ar, state) == 0
        after, s1 = snap(ar), down(state)
        check_tick(s0, s1, t)
        r = check_step(before, after, scalars(s1), what=f"n={n} t={t}")
    print(f"n={n}: error / bound at t=5: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def test_dev_launch_without_tick_uses_the_corrections_that_are_there():
    n = 2052
    ar, state = arena(n, seed=7), new_state()
    for _ in range(2):
        assert launch_dev(ar, state) == 0
    before, s0 = snap(ar), down(state)
    assert launch_dev(ar, state, tick=0) == 0
    after, s1 = snap(ar), down(state)
    assert same_bits(s0, s1)
    assert s1[0] == 2.0
    check_step(before, after, scalars(s0), what="tick=0")


@pytest.mark.parametrize("gs,lr", [(0.125, LRF), (3.0, LRF), (1.0, 0.0), (0.0, LRF)])
def test_dev_grad_scale_and_learning_rate_come_from_dev_state(gs, lr):
    n = 2052
    ar, state = arena(n, seed=11), new_state()
    assert launch_dev(ar, state) == 0                       # moments that are not zero
    state[4:6].copy_(torch.tensor([float(lr), gs], dtype=torch.float32))
    before, s0 = snap(ar), down(state)
    assert launch_dev(ar, state) == 0
    after, s1 = snap(ar), down(state)
    check_tick(s0, s1, 2)
    check_step(before, after, scalars(s1), what=f"gs={gs} lr={lr}")
    moved = before["g"] != 0
    assert moved.sum() > n // 2
    if lr == 0.0:
        assert same_bits(before["p"], after["p"])
        assert (before["m"][moved] != after["m"][moved]).all()
        squares = np.abs(before["g"]) > 1e-15                    # (1e-30)^2 is zero in fp32: v stays zero there
        assert (before["v"][squares] != after["v"][squares]).all()
    else:
        assert not same_bits(before["p"], after["p"])


N_CLEAR = 4100                              # three blocks, the last with a single float4
EIGHT = [(4, 36), (100, 100), (516, 1020), (1020, 1500), (2044, 2052), (2500, 2504), (3000, 3076), (4000, N_CLEAR)]


@pytest.mark.parametrize("case", ["null", "none", "all", "eight"])
def test_dev_clear_ranges(case):
    """g is exactly zero inside the ranges and keeps its bits outside; p, m, v meet the bounds everywhere, so a cleared
    gradient never hides an update that was not made.  Boundaries inside blocks (2048 elements), an empty range, two
    adjacent ones, one from the second float4, one up to n."""
    n = N_CLEAR
    spans = {"null": None, "none": [], "all": [(0, n)], "eight": EIGHT}[case]
    ar, state = arena(n, seed=13), new_state()
    ar["g"] = Buf(data=np.where(grad_mixture(14, n) == 0, np.float32(1e-4), grad_mixture(14, n)).astype(np.float32))      # no zeros
    mask = np.zeros(n, dtype=bool)
    for a, b in spans or []:
        mask[a:b] = True
    if case == "eight":
        assert all(a % BLOCK and b % BLOCK and a % 1024 and (b % 1024 or b == n) for a, b in EIGHT) and 0 < mask.sum() < n
    before, s0 = snap(ar), down(state)
    assert launch_dev(ar, state, clear=None if spans is None else ranges(spans)) == 0
    after, s1 = snap(ar), down(state)
    check_tick(s0, s1, 1)
    check_step(before, after, scalars(s1), cleared=mask, what=case)
    # the next step reads the cleared gradients: the moments decay there and follow the gradient elsewhere
    before, s0 = after, s1
    assert launch_dev(ar, state) == 0
    after, s1 = snap(ar), down(state)
    check_step(before, after, scalars(s1), what=case + ", second step")


@pytest.mark.parametrize("tick", [1, 0])
def test_dev_skip_word_stops_everything(tick):
    n = 2052
    ar, state = arena(n, seed=17), new_state()
    assert launch_dev(ar, state) == 0
    word = torch.tensor([2, 0, 0, 0], dtype=torch.uint8, device=DEV)          # a uint32 holding 2
    before, s0 = snap(ar), down(state)
    assert launch_dev(ar, state, skip=word, clear=ranges([(0, n)]), tick=tick) == 0
    unchanged(before, snap(ar), "skip word set")
    assert same_bits(s0, down(state))
    word.zero_()
    assert launch_dev(ar, state, skip=word, clear=ranges([(0, n)]), tick=tick) == 0
    after, s1 = snap(ar), down(state)
    if tick:
        check_tick(s0, s1, 2)
    else:
        assert same_bits(s0, s1)
    check_step(before, after, scalars(s1), cleared=np.ones(n, dtype=bool), what="skip word clear")
    assert not same_bits(before["p"], after["p"])


def test_dev_refuses_bad_arguments_and_changes_nothing():
    n = 64
    ar, state = arena(n, seed=19), new_state()
    before, s0 = snap(ar), down(state)
    calls = {
        "n = 0": dict(n=0), "n = 2": dict(n=2), "n = 6": dict(n=6),
        "misaligned p": dict(n=n - 4, offsets=(4, 0, 0, 0)), "misaligned g": dict(n=n - 4, offsets=(0, 8, 0, 0)),
        "misaligned m": dict(n=n - 4, offsets=(0, 0, 4, 0)), "misaligned v": dict(n=n - 4, offsets=(0, 0, 0, 12)),
        "clear->n = 9": dict(clear=ranges([(0, 4)], n=9)), "clear->n = -1": dict(clear=ranges([(0, 4)], n=-1)),
        "range past n": dict(clear=ranges([(0, n + 4)])), "range before 0": dict(clear=ranges([(-4, 8)])),
        "lo > hi": dict(clear=ranges([(8, 4)])),
        "lo % 4": dict(clear=ranges([(2, 8)])), "hi % 4": dict(clear=ranges([(0, 6)])),
        "second range bad": dict(clear=ranges([(0, 4), (8, n + 4)])),
    }
    for what, kw in calls.items():
        assert launch_dev(ar, state, **kw) == EINVAL, what
    L = _lib.lib()
    for i in range(4):                                                                   # a null buffer, no state
        ptrs = [None if j == i else ar[k].ptr for j, k in enumerate("pgmv")]
        assert L.dvae_adam_flat_dev(*ptrs, n, 0.9, 0.999, 1e-8, state.data_ptr(), None, None, 1, st()) == EINVAL
    assert L.dvae_adam_flat_dev(*(ar[k].ptr for k in "pgmv"), n, 0.9, 0.999, 1e-8, None, None, None, 1, st()) == EINVAL
    unchanged(before, snap(ar), "refused calls")
    assert same_bits(s0, down(state))
    assert launch_dev(ar, state, clear=ranges([(0, 4), (60, 64)])) == 0                  # ... and a good one is taken
    check_tick(s0, down(state), 1)


# ------------------------------------------------------------------ dvae_adam_flat (host scalars, scalar tail)
@pytest.mark.parametrize("n", [1, 3, 5, 1027, 4194304 + 1028 + 3])
def test_host_scalar_entry_point(n):
    """float4 body plus the scalar tail of n % 4 elements; the large size is one full grid-stride sweep (4096 blocks), a
    ragged second one and a tail of three.  step = 1 from zero moments, then step = 7 on what that left; grad_scale 0.5."""
    ar = arena(n, seed=23 + n % 100)
    for step in (1, 7):
        before = snap(ar)
        rc = _lib.lib().dvae_adam_flat(*(ar[k].ptr for k in "pgmv"), n, float(LRF), float(B1F), float(B2F), float(EPSF), 0.5,
                                       step, st())
        assert rc == 0
        after = snap(ar)
        bc1, bc2s = (np.float32(x) for x in bias_corrections(float(B1F), float(B2F), step))      # as the entry point does
        r = check_step(before, after, (LRF, B1F, B2F, EPSF, np.float32(0.5), bc1, bc2s), what=f"n={n} step={step}")
        if (np.abs(before["g"]) >= 1e-8).any():
            assert not same_bits(before["p"], after["p"])
    print(f"n={n}: error / bound at step 7: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def test_host_scalar_entry_point_refuses():
    ar = arena(8, seed=29)
    before = snap(ar)
    L, ptrs = _lib.lib(), [ar[k].ptr for k in "pgmv"]
    assert L.dvae_adam_flat(*ptrs, 0, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, st()) == EINVAL
    assert L.dvae_adam_flat(*ptrs, 8, 1e-3, 0.9, 0.999, 1e-8, 1.0, 0, st()) == EINVAL
    assert L.dvae_adam_flat(ptrs[0] + 4, *ptrs[1:], 4, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, st()) == EINVAL
    assert L.dvae_adam_flat(None, *ptrs[1:], 8, 1e-3, 0.9, 0.999, 1e-8, 1.0, 1, st()) == EINVAL
    unchanged(before, snap(ar), "refused calls")


# ------------------------------------------------------------------ FlatAdam on the device
SHAPES = [("p0", (37, 5)), ("p1", (1001,)), ("p2", (4, 4)), ("p3", (5000,))]      # offsets 0, 188, 1192, 1208: not block multiples
CUTS = [0, 500, 1236, 2500, 5004, 6208]                                        # multiples of 4, none of 32 inside
MIDDLE = (500, 1236)                                                           # holds the end of p1 (1192)


class Transposed:
    """A layout object as the model is one: p0 is stored [37][5], the checkpoint holds it [5][37]."""

    def reference_layout(self, name, t):
        return t.t() if name == "p0" else t

    def storage_layout(self, name, t):
        return t.t() if name == "p0" else t


def make_opt(layout=None, values=None):
    ps = []
    for i, (name, shape) in enumerate(SHAPES):
        x = torch.from_numpy(params(40 + i, int(np.prod(shape)))).view(shape) if values is None else values[name]
        ps.append((name, torch.nn.Parameter(x.detach().clone().to(DEV))))
    opt = FlatAdam(ps, lr=LR, layout=layout)
    assert opt.numel == CUTS[-1] and [opt.offsets[n] for n, _ in SHAPES] == [0, 188, 1192, 1208]
    return opt


def feed(opt, seed):
    """This step's gradients, from the mixture, written into p.grad.  Returns them as one float64 vector per parameter."""
    out = []
    for i, p in enumerate(opt.params):
        g = grad_mixture(1000 * seed + i, p.numel())
        p.grad.copy_(torch.from_numpy(g).view(p.shape))
        if getattr(p, "_dvae_grad_store_first", False):
            p._dvae_sf_writes = 1                      # written once, as the backward pass of a step does
        out.append(g.astype(np.float64))
    return out


def padding(opt):
    pad = np.ones(opt.numel, dtype=bool)
    for n, p in zip(opt.names, opt.params):
        pad[opt.offsets[n]:opt.offsets[n] + p.numel()] = False
    return pad


def zero_mask(opt, lo=0, hi=None):
    mask = np.zeros(opt.numel, dtype=bool)
    if opt.fold_zero_grad:
        for a, b in opt._zero_ranges:
            mask[max(a, lo):min(b, opt.numel if hi is None else hi)] = True
    return mask


@pytest.fixture(scope="module")
def twenty_steps():
    """20 steps, a different gradient draw each, every step compared with one reference step from the buffers downloaded
    before it; torch.optim.Adam on float64 copies is fed the same gradients."""
    opt = make_opt()
    ref = [torch.nn.Parameter(p.detach().cpu().double().clone()) for p in opt.params]
    topt = torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=EPS)
    pad = padding(opt)
    res = {"ratios": [], "p_literal": [], "pad_nonzero": 0, "t": []}
    for t in range(1, 21):
        gs = feed(opt, t)
        for r, g in zip(ref, gs):
            r.grad = torch.from_numpy(g).view(r.shape)
        topt.step()
        before = flat(opt)
        opt.step()
        after, s1 = flat(opt), down(opt.dev_state)
        res["t"].append((float(s1[0]), opt.t))
        res["pad_nonzero"] += sum(int(bits(after[k][pad]).any()) for k in "pgmv")
        # every check of one step but the 12-rounding bound of p, which gets a test of its own (module docstring)
        res["ratios"].append(check_step(before, after, scalars(s1), zero_mask(opt), "tol_p_cancel", f"step {t}"))
        b = one_step_bounds(before["p"], before["g"], before["m"], before["v"], *scalars(s1))
        res["p_literal"].append(worst_ratio(after["p"], b["ref_p"], b["tol_p"])[0])
        WORST.record("p", res["p_literal"][-1])
    res["p"] = np.concatenate([down(p.detach()).reshape(-1) for p in opt.params]).astype(np.float64)
    res["p_torch"] = np.concatenate([r.detach().numpy().reshape(-1) for r in ref])
    return res


def test_flat_adam_twenty_steps_meet_the_one_step_bounds(twenty_steps):
    """exp_avg and exp_avg_sq over the whole flat buffers, padding included, at every step; p against the bound that carries
    the absolute error of m' through the division (tests/adam_ref.py, `tol_p_cancel`); the gradient cleared; the step
    counter; the padding of all four buffers exactly zero."""
    res = twenty_steps
    assert res["t"] == [(float(t), t) for t in range(1, 21)]
    assert res["pad_nonzero"] == 0
    worst = {k: max(r[k] for r in res["ratios"]) for k in "mvp"}
    print("20 steps, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " (p: cancellation form)")
    assert max(worst.values()) <= 1.0


def test_flat_adam_twenty_steps_p_meets_the_twelve_rounding_bound(twenty_steps):
    """|p' - ref| <= eps32 |ref| + 12 eps32 |u| at every one of the 20 steps, over the whole flat buffer.

    The 12 counts m' = m + (g - m)(1 - b1) as four roundings relative to itself.  Where the gradient of an element flips
    sign and m' cancels (m = -106, g = 1e3: m' = 4.2) it keeps the absolute error of its terms, which the m bound allows,
    and an element with |p| < 1e-3 can then exceed this bound (the numpy fp32 restatement of tests/test_adam_ref.py does, by
    1.75 x, at one element-step of 124 160 of ITS gradient draw).  With the gradients drawn here neither the restatement
    nor the kernel gets there; if a changed draw does, the element will be one of those, and `tol_p_cancel` (asserted in
    the test above) is the bound that holds for it."""
    worst = max(twenty_steps["p_literal"])
    print(f"20 steps, worst p error / (eps32 |ref| + 12 eps32 |u|): {worst:.3f} per step: "
          + " ".join(f"{x:.2f}" for x in twenty_steps["p_literal"]))
    assert worst <= 1.0, worst


def test_flat_adam_twenty_steps_end_where_torch_adam_in_float64_ends(twenty_steps):
    p, ref = twenty_steps["p"], twenty_steps["p_torch"]
    tol = 20 * (EPS32 * np.abs(ref) + 3e-5 * LR)
    r, i = worst_ratio(p, ref, tol)
    print(f"20 steps against torch.optim.Adam(float64): worst error / bound {r:.3f}")
    assert r <= 1.0, (f"element {i}: {p[i]!r} against {ref[i]!r}; allowed per step: eps32 |p| = {EPS32 * abs(ref[i]):.3g} "
                      f"(storage rounding of p) + 3e-5 lr = {3e-5 * LR:.3g} (float32 hyperparameters and arithmetic)")


def configure(opt, variant):
    if variant == "store_first":
        opt.set_store_first(["p1"])
        assert opt._zero_ranges == [(0, 188), (1192, opt.numel)]
    elif variant == "no_fold":
        opt.fold_zero_grad = False
    return opt


@pytest.mark.parametrize("variant", ["fold", "store_first", "no_fold"])
def test_sharded_step_equals_full_step_bit_for_bit(variant):
    """step_range over a partition of the flat buffers — the whole sharded (rs_ag) optimizer — against one step(), pieces
    in order and reordered behind the ticking one."""
    pieces = list(zip(CUTS[:-1], CUTS[1:]))
    assert all(c % 4 == 0 and c % 32 for c in CUTS[1:-1])
    for order in ([0, 1, 2, 3, 4], [0, 3, 1, 4, 2]):
        a, b = configure(make_opt(), variant), configure(make_opt(), variant)
        for step in range(1, 4):
            feed(a, step)
            feed(b, step)
            a.step(0.5)
            for j, k in enumerate(order):
                b.step_range(*pieces[k], 0.5, tick=(j == 0))
            fa, fb = flat(a), flat(b)
            for k in "pmvg":
                assert same_bits(fa[k], fb[k]), (variant, order, step, k)
            assert a.t == b.t == step
        assert not bits(fa["g"][zero_mask(a)]).any() and (variant == "fold" or fa["g"][~zero_mask(a)].any())


@pytest.mark.parametrize("variant", ["fold", "store_first", "no_fold"])
def test_one_step_range_touches_only_its_piece(variant):
    lo, hi = MIDDLE
    opt = configure(make_opt(), variant)
    feed(opt, 1)
    opt.step(0.5)                                        # moments that are not zero, everywhere
    feed(opt, 1)
    before = flat(opt)
    opt.step_range(lo, hi, 0.5, tick=True)
    after, s1 = flat(opt), down(opt.dev_state)
    assert s1[0] == 2.0 and s1[5] == 0.5
    for k in "pmvg":
        assert same_bits(before[k][:lo], after[k][:lo]) and same_bits(before[k][hi:], after[k][hi:]), (variant, k)
    cut = lambda d: {k: x[lo:hi] for k, x in d.items()}
    cleared = zero_mask(opt, lo, hi)[lo:hi]
    assert cleared.sum() == {"fold": hi - lo, "store_first": hi - 1192, "no_fold": 0}[variant]
    check_step(cut(before), cut(after), scalars(s1), cleared, what=f"{variant} [{lo}, {hi})")
    assert not same_bits(before["p"][lo:hi], after["p"][lo:hi])


@pytest.mark.parametrize("layout", [None, Transposed()], ids=["plain", "permuting"])
def test_checkpoint_round_trip_continues_bit_for_bit(layout):
    a = make_opt(layout)
    for step in range(1, 5):
        feed(a, step)
        a.step()
    sd = a.state_dict()
    if layout is not None:
        assert tuple(sd["exp_avg"]["p0"].shape) == (5, 37)
    b = make_opt(layout, values={n: p.detach().cpu() for n, p in zip(a.names, a.params)})
    b.load_state_dict(sd)
    assert b.t == 4
    feed(a, 5)
    feed(b, 5)
    a.step()
    b.step()
    fa, fb = flat(a), flat(b)
    for k in "pmvg":
        assert same_bits(fa[k], fb[k]), k
    assert a.t == b.t == 5
    assert same_bits(down(a.dev_state), down(b.dev_state))


def test_zero_grad_scale_is_honoured_and_none_keeps_the_last():
    """grad_scale = 0.0 used to become 1.0 silently.  It is a scale: the moments decay, p moves by the decayed first moment."""
    opt = make_opt()
    for step in (1, 2):
        feed(opt, step)
        opt.step()
    for t, gs in ((3, 0.0), (4, None)):
        feed(opt, t)
        before = flat(opt)
        opt.step(grad_scale=gs)
        after, s1 = flat(opt), down(opt.dev_state)
        assert s1[0] == float(t) and s1[5] == 0.0
        check_step(before, after, scalars(s1), zero_mask(opt), what=f"grad_scale={gs}")
        live = before["m"] != 0
        assert live.sum() > opt.numel // 2
        assert np.abs(after["m"][live]).max() < np.abs(before["m"][live]).max()
        assert (np.abs(after["m"][live]) < np.abs(before["m"][live])).all()
        assert (after["v"][before["v"] > 1e-30] < before["v"][before["v"] > 1e-30]).all()
        assert not same_bits(before["p"], after["p"])
    opt.step(grad_scale=1.0)
    assert float(opt.dev_state[5]) == 1.0


def test_scalar_sender_keeps_every_pair_through_the_ring_wrap():
    """optim.ScalarSender on its own: 40 sends of 40 distinct pairs to one 2-float device buffer, a clone of the buffer enqueued
    behind each, ONE synchronise at the end.  The ring has 16 pinned slots, so send 17 reuses the slot of send 1 while copies
    are still in flight: a slot overwritten before its copy had read it would show as a later pair in an earlier clone."""
    from dvae_amd.optim import ScalarSender
    sender, buf = ScalarSender(), torch.zeros(2, device=DEV, dtype=torch.float32)
    assert sender.SLOTS == 16 and sender.WIDTH >= 8
    pairs = [(float(i) + 0.5, -3.0 * i - 1.0) for i in range(40)]
    assert len(set(pairs)) == 40
    clones = []
    for pair in pairs:
        sender.send([(buf[0:2], pair)])
        clones.append(buf.clone())
    torch.cuda.synchronize()
    got = [tuple(c.tolist()) for c in clones]
    assert got == pairs, [(i, g, p) for i, (g, p) in enumerate(zip(got, pairs)) if g != p]
