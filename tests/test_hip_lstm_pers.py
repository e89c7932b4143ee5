"""W_hh-resident persistent LSTM recurrence (csrc/lstm_pers.hip; nn.LSTM at /root/reference/model/disentangled_vae.py:172,193).

One launch walks all T frames; workgroups hand h[t] / dG[t] to each other through flags.  Checked here, through the C ABI:
  * against the one-launch-per-frame kernels on the same inputs (same arithmetic, other summation order), every shape
    class: H = 512 / 1024, 16- and 32-row workgroups, ragged N, reverse direction, bf16 and fp32 state storage;
  * hand-offs under UNEVEN load (a second stream hammering HBM meanwhile), repeated, every word compared;
  * a 10 000-frame soak;
  * the bounded spin: a workgroup that never publishes makes every waiter give up inside the timeout and
    dvae_lstm_pers_check report DVAE_ELAUNCH; the next launch on the same workspace is clean.
(The bf16 oracle comparison of the same path is tests/test_hip_bf16.py::test_lstm_layer_bf16, which runs LstmLayerFn.)"""
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture()
def env():
    import dvae_amd  # noqa: F401
    from dvae_amd import _lib, ops
    from dvae_amd.derived import lstm_local
    ops.set_compute_dtype("bf16")
    yield _lib, ops, lstm_local
    ops.set_compute_dtype(ops.DEFAULT_COMPUTE_DTYPE)


class Layer:
    """Buffers of one LSTM layer-direction for direct dvae_lstm_seq_fwd / _bwd calls."""

    def __init__(self, env, T, N, H, s16, reverse=0, seed=0):
        _lib, ops, lstm_local = env
        self.env, self.T, self.N, self.H, self.s16, self.reverse = env, T, N, H, s16, reverse
        g = torch.Generator(device="cuda").manual_seed(seed)
        f = dict(device="cuda", dtype=torch.float32)
        sdt = torch.bfloat16 if s16 else torch.float32
        self.w_hh = (torch.rand(4 * H, H, generator=g, **f) * 2 - 1) / H ** 0.5
        w_ih = torch.zeros(4 * H, 64, **f)
        b = torch.zeros(4 * H, **f)
        self.der = lstm_local(w_ih, self.w_hh, b, b, _lib.MODE_BF16)
        self.gates0 = (torch.rand(T * N, 4 * H, generator=g, **f) * 2 - 1)
        self.dh = (torch.rand(T * N, H, generator=g, **f) * 2 - 1) * 0.1
        self.gates = torch.empty(T * N, 4 * H, **f)
        self.h = torch.empty(T * N, H, device="cuda", dtype=sdt)
        self.c = torch.empty(T * N, H, **f)
        self.dg = torch.empty(T * N, 4 * H, device="cuda", dtype=sdt)
        self.dc = torch.empty(N, H, **f)

    def dirs(self, bwd, pers, timeout_us=0):
        _lib, ops, _ = self.env
        ptr = _lib.ptr
        d = (_lib.LstmDir * 1)()
        d[0].gates, d[0].c_all = ptr(self.gates), ptr(self.c)
        d[0].w_hh = ptr(self.der.w_hh_t if bwd else self.w_hh)
        d[0].w_packed = ptr(self.der.pack_b if bwd else self.der.pack_f)
        d[0].h_out, d[0].dh_out, d[0].dgates, d[0].dc_ws = ptr(self.h), ptr(self.dh), ptr(self.dg), ptr(self.dc)
        d[0].reverse, d[0].packed_mode, d[0].step_shift, d[0].state_bf16 = self.reverse, _lib.MODE_BF16, 0, int(self.s16)
        if pers:
            d[0].pers_ws, d[0].pers_timeout_us = ptr(ops.lstm_pers_workspace("cuda")), timeout_us
        return d

    def run(self, pers, timeout_us=0):
        """forward + backward; returns clones of (gates, c, h, dgates)"""
        _lib, ops, _ = self.env
        L, st = _lib.lib(), _lib.stream()
        self.gates.copy_(self.gates0)
        self.h.fill_(float("nan"))
        self.dg.fill_(float("nan"))
        _lib.check(L.dvae_lstm_seq_fwd(self.dirs(False, pers, timeout_us), 1, self.T, self.N, self.H, self.H, st), "fwd")
        _lib.check(L.dvae_lstm_seq_bwd(self.dirs(True, pers, timeout_us), 1, self.T, self.N, self.H, self.H, st), "bwd")
        if pers:
            ops.lstm_pers_check()
        return [t.float().clone() for t in (self.gates, self.c, self.h, self.dg)]


def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def compare(got, ref, tag):
    # same products, another fp32 summation order; the state / gate gradients are ROUNDED to bf16 for the next frame on
    # both sides, so a last-bit difference in front of a rounding can flip one bf16 ulp (2^-8) of single elements:
    # relative L2 over the tensor stays tiny, no element may be further away than a few bf16 ulps
    for name, g, r in zip(("gates", "c", "h", "dgates"), got, ref):
        assert torch.isfinite(g).all(), f"{tag}: {name} not finite"
        e = rel_l2(g, r)
        assert e < 2e-3, f"{tag}: {name} rel-L2 {e:.3e}"
        worst = float((g - r).abs().max())
        scale = float(r.abs().max())
        assert worst <= 2e-2 * scale, f"{tag}: {name} max |diff| {worst:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("H,T,N,s16,reverse", [
    (512, 6, 128, True, 0),      # 16 x 8 = 128 workgroups of 16 rows
    (512, 5, 256, True, 0),      # 16 x 16 = 256 workgroups
    (1024, 8, 128, True, 0),     # configs[1]/[4] per-GPU shape: 32 x 8 workgroups of 16 rows
    (1024, 6, 256, True, 0),     # configs[2]: 32 x 8 workgroups of 32 rows
    (1024, 4, 17, True, 0),      # ragged: 2 row blocks, the second with one live row
    (512, 3, 40, False, 0),      # fp32 state storage
    (1024, 5, 128, False, 1),    # reverse direction, fp32 state storage
    (1024, 1, 128, True, 0),     # a single frame: nothing is ever handed over
])
def test_persistent_matches_frame_kernels(env, H, T, N, s16, reverse):
    _lib, ops, _ = env
    assert ops.lstm_persistent_usable(N, H, _lib.MODE_BF16)
    lay = Layer(env, T, N, H, s16, reverse, seed=H + T + N)
    ref = lay.run(pers=False)
    got = lay.run(pers=True)
    compare(got, ref, f"H={H} T={T} N={N} s16={s16} rev={reverse}")
    # the same exchange slots again with OTHER data (another layer, the next training step): nothing of the previous
    # launches may be read back from a cache
    lay.gates0.neg_().mul_(0.7)
    lay.dh.mul_(-1.3)
    ref = lay.run(pers=False)
    got = lay.run(pers=True)
    compare(got, ref, f"second launch with other data, H={H} T={T} N={N}")


@pytest.mark.parametrize("H,T,N,reverse", [(1024, 8, 128, 0), (512, 6, 128, 0), (1024, 5, 40, 1), (512, 1, 128, 0),
                                            (1024, 3, 17, 0),
                                            # H = 512 forward: lstm_pers_fwd_x3h (8 units x 32 rows), ragged row groups too
                                            (512, 5, 40, 1), (512, 3, 17, 0), (512, 7, 97, 1)])
def test_persistent_fp32x3_forward_fp32_backward_match_frame_kernels(env, H, T, N, reverse):
    """The default arithmetic: the forward recurrence on three resident bf16 planes of W_hh (h handed over as three
    planes, fp32 results); the backward one on three resident planes too (dG handed over in fp32, split by the consumer)
    or on resident fp32 fragments.  Against the per-frame
    kernels of the same arithmetic only the fp32 summation order differs; the persistent backward also leaves the bias
    gradient (column sums of dG)."""
    _lib, ops, lstm_local = env
    L, st, ptr = _lib.lib(), _lib.stream(), _lib.ptr
    X3, F32 = _lib.MODE_F32X3, _lib.MODE_F32
    assert ops.lstm_persistent_usable(N, H, X3) and ops.lstm_persistent_usable(N, H, X3, bwd=True)
    assert ops.lstm_persistent_usable(N, H, F32, bwd=True) and not ops.lstm_persistent_usable(N, H, F32)
    g = torch.Generator(device="cuda").manual_seed(H + T + N)
    f = dict(device="cuda", dtype=torch.float32)
    w_hh = (torch.rand(4 * H, H, generator=g, **f) * 2 - 1) / H ** 0.5
    der = lstm_local(torch.zeros(4 * H, 64, **f), w_hh, torch.zeros(4 * H, **f), torch.zeros(4 * H, **f), X3)
    gates0 = torch.rand(T * N, 4 * H, generator=g, **f) * 2 - 1
    dh = (torch.rand(T * N, H, generator=g, **f) * 2 - 1) * 0.1
    pack_b32 = torch.empty(4 * H * H, **f)          # fp32 fragments of W_hh for the backward pass (der.pack_b: three planes)
    _lib.check(L.dvae_lstm_pack_w(ptr(w_hh), None, ptr(pack_b32), H, st), "pack")
    outs = []
    for pers, bmode in ((False, F32), (True, F32), (True, X3)):
        gates, h, c = gates0.clone(), torch.full((T * N, H), float("nan"), **f), torch.empty(T * N, H, **f)
        dg, dc, db = torch.full((T * N, 4 * H), float("nan"), **f), torch.empty(N, H, **f), torch.zeros(2, 4 * H, **f)
        d = (_lib.LstmDir * 1)()
        d[0].gates, d[0].c_all, d[0].h_out, d[0].w_hh, d[0].w_packed = ptr(gates), ptr(c), ptr(h), ptr(w_hh), ptr(der.pack_f)
        d[0].reverse, d[0].packed_mode = reverse, X3
        ws = ops.lstm_pers_workspace("cuda")
        if pers:
            d[0].pers_ws = ptr(ws)
        _lib.check(L.dvae_lstm_seq_fwd(d, 1, T, N, H, H, st), "fwd")
        b = (_lib.LstmDir * 1)()
        b[0].gates, b[0].c_all, b[0].w_hh = ptr(gates), ptr(c), ptr(der.w_hh_t)
        b[0].w_packed = ptr(der.pack_b if bmode == X3 else pack_b32)
        b[0].dh_out, b[0].dgates, b[0].dc_ws, b[0].reverse, b[0].packed_mode = ptr(dh), ptr(dg), ptr(dc), reverse, bmode
        if pers:
            b[0].pers_ws, b[0].dbias_ih, b[0].dbias_hh = ptr(ws), ptr(db[0]), ptr(db[1])
        _lib.check(L.dvae_lstm_seq_bwd(b, 1, T, N, H, H, st), "bwd")
        ops.lstm_pers_check()
        outs.append((gates, c, h, dg, db))
    want = outs[0][3].double().sum(0)
    for which in (1, 2):          # persistent fp32 backward, persistent fp32x3 backward (dG split by the consumer)
        for name, a, b in zip(("gates", "c", "h", "dgates"), outs[which], outs[0]):
            assert torch.isfinite(a).all(), name
            err = float((a - b).abs().max())
            assert err <= 2e-5 * float(b.abs().max()), f"{name} ({which}): max |diff| {err:.3e}"
        for k in range(2):
            err = float((outs[which][4][k].double() - want).abs().max())
            assert err <= 1e-4 * float(want.abs().max()), f"bias gradient {k} ({which}): {err:.3e}"


def _x3_pass(env, H, T, N, pers, seed=0):
    """forward + backward of one layer in the default arithmetic (fp32x3) through the C ABI; pers: the W_hh-resident
    launches (H = 1024 backward: the k-split kernel with its second, partial-tile hand-off; H = 512: 16-row tiles)."""
    _lib, ops, lstm_local = env
    L, st, ptr = _lib.lib(), _lib.stream(), _lib.ptr
    X3 = _lib.MODE_F32X3
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    f = dict(device="cuda", dtype=torch.float32)
    w_hh = (torch.rand(4 * H, H, generator=g, **f) * 2 - 1) / H ** 0.5
    der = lstm_local(torch.zeros(4 * H, 64, **f), w_hh, torch.zeros(4 * H, **f), torch.zeros(4 * H, **f), X3)
    gates = torch.rand(T * N, 4 * H, generator=g, **f) * 2 - 1
    dh = (torch.rand(T * N, H, generator=g, **f) * 2 - 1) * 0.1
    h, c = torch.full((T * N, H), float("nan"), **f), torch.empty(T * N, H, **f)
    dg, dc, db = torch.full((T * N, 4 * H), float("nan"), **f), torch.empty(N, H, **f), torch.zeros(2, 4 * H, **f)
    ws = ops.lstm_pers_workspace("cuda")
    d = (_lib.LstmDir * 1)()
    d[0].gates, d[0].c_all, d[0].h_out, d[0].w_hh, d[0].w_packed = ptr(gates), ptr(c), ptr(h), ptr(w_hh), ptr(der.pack_f)
    d[0].packed_mode = X3
    b = (_lib.LstmDir * 1)()
    b[0].gates, b[0].c_all, b[0].w_hh, b[0].w_packed = ptr(gates), ptr(c), ptr(der.w_hh_t), ptr(der.pack_b)
    b[0].dh_out, b[0].dgates, b[0].dc_ws, b[0].packed_mode = ptr(dh), ptr(dg), ptr(dc), X3
    if pers:
        d[0].pers_ws = b[0].pers_ws = ptr(ws)
        b[0].dbias_ih, b[0].dbias_hh = ptr(db[0]), ptr(db[1])
    _lib.check(L.dvae_lstm_seq_fwd(d, 1, T, N, H, H, st), "fwd")
    _lib.check(L.dvae_lstm_seq_bwd(b, 1, T, N, H, H, st), "bwd")
    if pers:
        ops.lstm_pers_check()
    return gates, c, h, dg


@pytest.mark.parametrize("H,T,N", [(1024, 96, 128), (512, 96, 128), (1024, 64, 97)])
def test_fp32x3_handoffs_under_uneven_load(env, H, T, N):
    """The default-arithmetic recurrences — at H = 1024 the k-split backward kernel with TWO hand-offs per frame (dG fragments,
    then the partial dh tiles between the four k-quarter workgroups of a block), at H = 512 the 16-row tiles — while a second
    stream streams 0 .. 4 GiB through HBM: every output word against the per-frame kernels, every round, and bit-for-bit
    against the first persistent run (the partial tiles are summed in a fixed order: no run-to-run noise).
    (scripts/x3_handoff_stress.py is the long form: hundreds of rounds, and it says which frame / rows went wrong.  It is what
    showed the 16-row FORWARD form failing 5-17 % of its rounds — that form is not in the product library.)"""
    ref = _x3_pass(env, H, T, N, pers=False)
    side = torch.cuda.Stream()
    a = torch.empty(1 << 28, device="cuda", dtype=torch.float32)
    b = torch.empty_like(a)
    first = None
    for rnd in range(15):
        with torch.cuda.stream(side):
            for _ in range(rnd % 5):
                b.copy_(a)
        got = _x3_pass(env, H, T, N, pers=True)
        for name, x, y in zip(("gates", "c", "h", "dgates"), got, ref):
            assert torch.isfinite(x).all(), (name, rnd)
            err = float((x - y).abs().max())
            assert err <= 2e-5 * float(y.abs().max()), f"{name}, round {rnd}: max |diff| {err:.3e}"
        if first is None:
            first = [t.clone() for t in got]
        else:
            for name, x, y in zip(("gates", "c", "h", "dgates"), got, first):
                assert torch.equal(x, y), f"{name}, round {rnd}: persistent runs differ bitwise"
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode,H,T,N", [("fp32x3", 1024, 64, 128),     # forward lstm_pers_fwd_x3<1024,8,2>, backward lstm_pers_bwd_x3k<1024>
                                         ("fp32x3", 512, 64, 128),      # forward lstm_pers_fwd_x3h<512> (8 units x 32 rows), backward lstm_pers_bwd_x3<512,0,1> (16 rows)
                                         ("bf16", 1024, 48, 256),       # lstm_pers_fwd/bwd_bf16<1024,2,2>: configs[2]
                                         ("bf16", 1024, 48, 128),       # lstm_pers_fwd/bwd_bf16<1024,1,0>: configs[4]'s per-GPU shape
                                         ("bf16", 512, 48, 128)])       # lstm_pers_fwd/bwd_bf16<512,1,0>
def test_every_product_persistent_kernel_300_rounds_under_foreign_traffic(env, mode, H, T, N):
    """the stress that lived in scripts/ only.  EVERY persistent recurrence kernel the product library
    dispatches at the benchmarked shapes, 300 rounds each, while a second stream streams 0 .. 4 GiB through HBM (a different
    amount every round: the launches meet the copies' kernel boundaries at different frames): every output word of every
    round against the per-frame kernels, and — the persistent kernels sum in a fixed order — bit for bit against the first
    persistent round.  (The 16-row FORWARD form of the fp32x3 kernel, which failed this stress on one box in round 4 and
    on one of five boxes in round 5, is not in the product library: DESIGN.md §4.2.)"""
    if mode == "fp32x3":
        run = lambda pers: _x3_pass(env, H, T, N, pers)
        tol = lambda y: 2e-5 * float(y.abs().max())
    else:
        lay = Layer(env, T, N, H, True, seed=11)
        run = lambda pers: lay.run(pers=pers)
        tol = lambda y: 2e-2 * float(y.abs().max())
    ref = [t.clone() for t in run(False)]
    side = torch.cuda.Stream()
    a = torch.empty(1 << 28, device="cuda", dtype=torch.float32)
    b = torch.empty_like(a)
    first = None
    for rnd in range(300):
        with torch.cuda.stream(side):
            for _ in range(rnd % 5):
                b.copy_(a)
        got = run(True)
        for name, x, y in zip(("gates", "c", "h", "dgates"), got, ref):
            assert torch.isfinite(x).all(), (name, rnd)
            err = float((x - y).abs().max())
            assert err <= tol(y), f"{mode} H={H}: {name}, round {rnd} ({rnd % 5} GiB): max |diff| {err:.3e}"
        if first is None:
            first = [t.clone() for t in got]
        else:
            for name, x, y in zip(("gates", "c", "h", "dgates"), got, first):
                assert torch.equal(x, y), f"{mode} H={H}: {name}, round {rnd}: persistent rounds differ bitwise"
    torch.cuda.synchronize()


def test_flag_epoch_advances_and_recycles_without_a_clearing_launch(env):
    """Round 5: nothing clears the flags in front of a persistent launch — a flag holds `epoch + frames published`, the epoch
    lives in the workspace (word 8 of the error record) and the last workgroup to finish advances it by T + 1.  (a) it advances
    by exactly that per launch; (b) once it has passed 2^30 the last workgroup zeroes every flag and starts again from 0, so
    nothing ever wraps: launches on both sides of that recycling stay correct — fp32x3 forward, both backward forms (the
    k-split one has two hand-offs) and the bf16 kernels, against the per-frame kernels."""
    _lib, ops, _ = env
    ws = ops.lstm_pers_workspace("cuda")
    off = _lib.lib().dvae_lstm_pers_err_word(ws.data_ptr()) - ws.data_ptr() + 8 * 4
    word = ws[off:off + 4].view(torch.int32)
    T = 300
    ref = [t.clone() for t in _x3_pass(env, 512, T, 128, pers=False, seed=7)]
    torch.cuda.synchronize()
    e0 = int(word.item())
    got = _x3_pass(env, 512, T, 128, pers=True, seed=7)
    torch.cuda.synchronize()
    e1 = int(word.item())
    assert e1 - e0 == 2 * (T + 1), (e0, e1)                            # one forward + one backward launch
    for name, x, y in zip(("gates", "c", "h", "dgates"), got, ref):
        assert float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()), name
    # 150 frames in front of the limit: the forward launch runs across it and recycles when it ends, the backward launch
    # starts from epoch 0 on zeroed flags
    word.fill_((1 << 30) - 150)
    torch.cuda.synchronize()
    got = _x3_pass(env, 512, T, 128, pers=True, seed=7)
    for name, x, y in zip(("gates", "c", "h", "dgates"), got, ref):
        assert float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()), f"{name} across the recycling"
    torch.cuda.synchronize()
    assert int(word.item()) == T + 1, int(word.item())                 # recycled by the forward launch, advanced by the backward one
    assert int(ws[:64 * 1024].view(torch.int32).max()) <= T + 1        # every flag started again from zero
    # the k-split backward (two hand-offs) and the bf16 kernels across a recycling of their own
    word.fill_((1 << 30) - 40)
    ref = [t.clone() for t in _x3_pass(env, 1024, 64, 128, pers=False, seed=8)]
    got = _x3_pass(env, 1024, 64, 128, pers=True, seed=8)
    for name, x, y in zip(("gates", "c", "h", "dgates"), got, ref):
        assert float((x - y).abs().max()) <= 2e-5 * float(y.abs().max()), f"H=1024 {name} across the recycling"
    word.fill_((1 << 30) - 40)
    lay = Layer(env, 48, 256, 1024, True, seed=12)
    compare(lay.run(pers=True), lay.run(pers=False), "bf16 across the recycling")
    torch.cuda.synchronize()
    assert int(word.item()) == 48 + 1, int(word.item())                # the forward launch recycled, the backward one advanced


def test_fp32x3_soak_3000_frames(env):
    """3 000 frames of the H = 1024 layer in one launch per pass (6 000 partial-tile exchanges per workgroup in the backward
    pass): no hang, no drift against the per-frame kernels."""
    T, N, H = 3000, 32, 1024
    ref = _x3_pass(env, H, T, N, pers=False, seed=4)
    got = _x3_pass(env, H, T, N, pers=True, seed=4)
    for name, x, y in zip(("gates", "c", "h", "dgates"), got, ref):
        assert torch.isfinite(x).all(), name
        assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()), name


def test_persistent_handoffs_under_uneven_load(env):
    """A second stream streams 1 GiB copies through HBM while the persistent launches run: hand-offs must not depend on
    timing.  Every output word is compared with the per-frame kernels' each round."""
    lay = Layer(env, 48, 256, 1024, True, seed=5)
    ref = lay.run(pers=False)
    side = torch.cuda.Stream()
    a = torch.empty(1 << 28, device="cuda", dtype=torch.float32)
    b = torch.empty_like(a)
    for rnd in range(6):
        with torch.cuda.stream(side):
            for _ in range(rnd):          # 0 .. 5 GiB of foreign traffic: the load differs round to round
                b.copy_(a)
        got = lay.run(pers=True)
        compare(got, ref, f"uneven load, round {rnd}")
    torch.cuda.synchronize()


def test_persistent_soak_10000_frames(env):
    """10 000 frames in ONE launch per pass (forward and backward): no hang, no drift against the per-frame kernels."""
    T, N, H = 10000, 32, 1024
    lay = Layer(env, T, N, H, True, seed=9)
    ref = lay.run(pers=False)
    t0 = time.time()
    got = lay.run(pers=True)
    dt = time.time() - t0
    compare(got, ref, "soak")
    # the last frames of each pass in particular (the end of a 10 000-deep dependency chain)
    for g, r in zip(got, ref):
        assert rel_l2(g[-N:], r[-N:]) < 5e-3 and rel_l2(g[:N], r[:N]) < 5e-3
    assert dt < 60.0, f"soak took {dt:.1f} s"


def test_bounded_spin_gives_up_and_reports(env):
    """Workgroup 3 never publishes: every waiter must give up within the timeout (here 20 ms), the launch must END, and
    dvae_lstm_pers_check must turn the sticky record into DVAE_ELAUNCH; the next launch on the workspace is clean."""
    _lib, ops, _ = env
    L, st = _lib.lib(), _lib.stream()
    lay = Layer(env, 16, 128, 1024, True, seed=3)
    ref = lay.run(pers=False)
    lay.gates.copy_(lay.gates0)
    d = lay.dirs(False, True, timeout_us=20000)
    torch.cuda.synchronize()
    t0 = time.time()
    _lib.check(L.dvae_lstm_pers_selftest(d, lay.T, lay.N, lay.H, lay.H, 3, st), "selftest")
    with pytest.raises(_lib.DvaeHipError, match="gave up"):
        ops.lstm_pers_check()
    dt = time.time() - t0
    assert dt < 5.0, f"the give-up took {dt:.2f} s"
    ops.lstm_pers_check()                   # the record is cleared once reported
    got = lay.run(pers=True)
    compare(got, ref, "after a timed-out launch")


@pytest.mark.parametrize("H,drop", [(512, 3), (512, 200), (1024, 77)])
def test_fp32x3_forward_gives_up_on_a_silent_producer(env, H, drop):
    """The same for the default arithmetic's forward kernels (H = 512: lstm_pers_fwd_x3h, every wave polls its own producers —
    each wave's give-up must end the whole workgroup; H = 1024: lstm_pers_fwd_x3): workgroup `drop` never publishes."""
    _lib, ops, lstm_local = env
    L, st, ptr = _lib.lib(), _lib.stream(), _lib.ptr
    T, N, X3 = 12, 128, _lib.MODE_F32X3
    ref = _x3_pass(env, H, T, N, False, seed=5)
    g = torch.Generator(device="cuda").manual_seed(1005)
    f = dict(device="cuda", dtype=torch.float32)
    w_hh = (torch.rand(4 * H, H, generator=g, **f) * 2 - 1) / H ** 0.5
    der = lstm_local(torch.zeros(4 * H, 64, **f), w_hh, torch.zeros(4 * H, **f), torch.zeros(4 * H, **f), X3)
    gates = torch.rand(T * N, 4 * H, generator=g, **f) * 2 - 1
    h, c = torch.zeros(T * N, H, **f), torch.zeros(T * N, H, **f)
    d = (_lib.LstmDir * 1)()
    d[0].gates, d[0].c_all, d[0].h_out, d[0].w_hh, d[0].w_packed = ptr(gates), ptr(c), ptr(h), ptr(w_hh), ptr(der.pack_f)
    d[0].packed_mode, d[0].pers_ws, d[0].pers_timeout_us = X3, ptr(ops.lstm_pers_workspace("cuda")), 20000
    torch.cuda.synchronize()
    t0 = time.time()
    _lib.check(L.dvae_lstm_pers_selftest(d, T, N, H, H, drop, st), "selftest")
    with pytest.raises(_lib.DvaeHipError, match="gave up"):
        ops.lstm_pers_check()
    assert time.time() - t0 < 5.0
    ops.lstm_pers_check()                   # the record is cleared once reported
    got = _x3_pass(env, H, T, N, True, seed=5)      # the next launches on the workspace are clean
    for name, a, b in zip(("gates", "c", "h", "dgates"), got, ref):
        err = float((a - b).abs().max())
        assert err <= 2e-5 * float(b.abs().max()), f"{name} after a timed-out launch: {err:.3e}"


def test_xcd_local_handoff_engages_only_where_row_groups_share_an_xcd(env):
    """Round 6: with a multiple of 8 row groups the workgroups of a row group share bid % 8, hence (round-robin dispatch) an
    XCD; they verify that at frame 1 and keep payload and flags in that XCD's L2.  The statistics word counts such launches:
    it must move for N = 128 (8 row groups of 16 rows) and must NOT for N = 40 (3 row groups) — and the results are those of the
    per-frame kernels either way (every other test of this file runs over the same workspace, local and write-through
    launches alternating)."""
    _lib, ops, _ = env
    if os.environ.get("DVAE_PERS_XCD_LOCAL", "1")[:1] == "0":
        pytest.skip("XCD-local hand-off switched off")
    n0 = ops.lstm_pers_local_launches()
    lay = Layer(env, 12, 40, 1024, True, seed=21)
    ref = lay.run(pers=False)
    compare(lay.run(pers=True), ref, "N = 40")
    assert ops.lstm_pers_local_launches() == n0, "3 row groups cannot be XCD-local"
    lay = Layer(env, 12, 128, 1024, True, seed=22)
    ref = lay.run(pers=False)
    compare(lay.run(pers=True), ref, "N = 128")
    n1 = ops.lstm_pers_local_launches()
    if n1 == n0:
        pytest.skip("workgroups were not dealt round-robin over the XCDs here: the launches stayed write-through (results checked)")
    assert n1 == n0 + 2                      # forward + backward
    lay = Layer(env, 4, 128, 1024, True, seed=23)      # too short: frames 1 .. T-4 only
    ref = lay.run(pers=False)
    compare(lay.run(pers=True), ref, "T = 4")


def test_workspace_size_contract(env):
    _lib, ops, _ = env
    L = _lib.lib()
    assert L.dvae_lstm_pers_ws_bytes(128, 1024) > 0 and L.dvae_lstm_pers_ws_bytes(256, 1024) > 0
    assert L.dvae_lstm_pers_ws_bytes(128, 64) == 0 and L.dvae_lstm_pers_ws_bytes(128, 768) == 0
    assert L.dvae_lstm_pers_ws_bytes(600, 1024) == 0           # would need more workgroups than CUs
    for N, H in ((128, 512), (256, 512), (512, 512), (128, 1024), (256, 1024), (17, 1024)):
        assert L.dvae_lstm_pers_ws_bytes(N, H) <= ops.lstm_pers_workspace("cuda").numel()


@pytest.mark.parametrize("mode,H,T,N", [("fp32x3", 512, 3, 40),      # three row groups of 16, the last ragged; dead slabs above
                                         ("bf16", 512, 3, 128)])     # eight full row groups, bf16 dgates
def test_selftest_pass_leaves_the_products_bias_slabs(env, mode, H, T, N):
    """selftest._pass drives the persistent backward launch as the product does — descriptors from ops._lstm_dir, bias
    gradients stored per row group into dbias_part — and returns the slabs: held by lstm_ref.bias_check against the
    launch's own dgates (float64 slab sum within gamma(T N + 16) sum|dG| + eps32 |s|; slabs of row groups the launch does
    not have exactly zero)."""
    import lstm_ref as R
    from dvae_amd import selftest
    _lib, ops, _ = env
    ops.set_compute_dtype(mode)
    m = _lib.COMPUTE_MODES[mode]
    if not (ops.lstm_persistent_usable(N, H, m) and ops.lstm_persistent_usable(N, H, m, bwd=True)):
        pytest.skip("no persistent launch for this shape on this device")
    out = selftest._pass(m, H, T, N, pers=True)
    assert len(out) == 5 and tuple(out[4].shape) == (_lib.PERS_BIAS_SLABS, 4 * H)
    dG = out[3].cpu().numpy().reshape(T, N, 4 * H)
    res = R.bias_check(dG, None, None, slabs=out[4].cpu().numpy())
    for k, (ratio, col) in res.items():
        print(f"{mode} H={H} T={T} N={N}: {k} ratio {ratio:.3f} (column {col})")
    assert set(res) == {"dbias_part", "dbias_part_zero_rows"}
    assert all(r <= 1.0 for r, _ in res.values()), res
    assert selftest._pass(m, H, T, N, pers=False)[4] is None           # the per-frame launches leave no bias gradient


def test_deployment_selftest_passes_here(env):
    """dvae_amd.selftest (the check to run on a new box before a long training run): every product persistent kernel against
    the per-frame kernels under foreign HBM traffic — a few rounds here; it must come back clean and leave the compute mode
    as it found the default."""
    from dvae_amd import selftest
    lines = []
    assert selftest.run(rounds=6, log=lines.append) == 0, "\n".join(lines)
    assert any("PASSED" in ln for ln in lines), lines
    # seven cases (five at T <= 64, two at the T = 512 of configs[4]): every one either ran clean or was reported as skipped
    ran = sum("0 bad rounds of" in ln for ln in lines)
    skipped = sum("(skipped)" in ln for ln in lines)
    assert ran + skipped == 7 and ran >= 1, lines
