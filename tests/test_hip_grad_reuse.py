"""Gradients of optimiser-owned parameters that one backward pass reaches more than once.

The training step (forward_full) runs every layer once, but the reference's own forward calls encode, decode and the
postnet twice each (disentangled_vae.py:250-279), and so does any caller of the class-level API.  Every use of such a weight
stores its k-split partial products into the parameter's one slab buffer, summed into `.grad` at the end of backward
(ops._defer_fold): the slabs of an earlier use must be summed before a later launch overwrites them (ops._claim_slabs).
Each op is applied 2 and 3 times to different inputs in one graph (loss sum_i <g_i, out_i>) with its parameters owned by a
FlatAdam, and `.grad` is read right after backward(), before any optimiser step.  A spy on ops._defer_fold makes sure the
deferred, split path really ran; a lost or doubled slab set would be an O(1) error."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_hip_kernels import close, persistent_lstm, rnd

pytestmark = pytest.mark.gpu
GRAD_REL = 5e-4           # test_hip_kernels.py: gradients against a CPU reference


@pytest.fixture(scope="module", params=["fp32x3", "fp32"])
def ops(request):
    import dvae_amd  # noqa: F401
    from dvae_amd import ops as o
    o.set_compute_dtype(request.param)
    yield o
    o.set_compute_dtype(o.DEFAULT_COMPUTE_DTYPE)


@pytest.fixture
def spy(monkeypatch):
    """[(gradient address, owned, nslab)] of every ops._defer_fold call"""
    from dvae_amd import ops as o
    seen = []
    real = o._defer_fold

    def defer(grad, owner, slab_ptr, stride, nslab, n=None):
        seen.append((grad.data_ptr(), owner is not None, nslab))
        return real(grad, owner, slab_ptr, stride, nslab, n)

    monkeypatch.setattr(o, "_defer_fold", defer)
    return seen


def split_uses(seen, params):
    """name -> number of owned k-split contributions (nslab > 1) the spy saw for that parameter's gradient"""
    at = {p.grad.data_ptr(): n for n, p in params.items() if p.grad is not None}
    out = {}
    for g, owned, nslab in seen:
        if owned and nslab > 1 and g in at:
            out[at[g]] = out.get(at[g], 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------- op cases
# Each case: init values of the parameters (fp32, CPU, in the layout the HIP op holds them), the op on the GPU, the same
# composition in plain torch, the input / output shapes, and the parameters whose weight gradient takes the deferred
# k-split path at this shape (checked through the spy, so a shape that stops splitting fails instead of passing vacuously).

class LinearCase:
    M, K, Nout = 2048, 512, 80                 # dW: 4 output tiles over K = 2048 rows -> split
    name = "linear"

    def init(self):
        return {"w": rnd(self.Nout, self.K, seed=2) * 0.05, "b": rnd(self.Nout, seed=3)}

    def shapes(self):
        return (self.M, self.K), (self.M, self.Nout)

    def hip(self, ops, P, x):
        return ops.LinearFn.apply(x, P["w"], P["b"], ops.ACT_RELU)

    def ref(self, P, x):
        return torch.relu(F.linear(x, P["w"], P["b"]))

    def split(self, ops, mode):
        return {"w"}

    compare = ("w", "b")


class ConvCase:
    """ConvBnActFn with G BatchNorm groups.  Smooth activations: a ReLU mask that flips on a pre-activation within round-off
    of zero moves single gradient elements by O(|dz|) between any two correct implementations, which is not what is tested
    here (the ReLU form of the same backward is the bn_bwd_from_y path that ACT_NONE takes too)."""
    N, T, Cin, Cout = 8, 64, 512, 512         # R = 512 rows: the model's convs at B = 8, T = 64 (one encode / decode)

    def __init__(self, G, act):
        self.G, self.act = G, act
        self.name = f"conv_g{G}"

    def init(self):
        return {"cw": (rnd(self.Cout, self.Cin, 5, seed=2) * 0.05).permute(2, 0, 1).contiguous(),   # packed [5][Cout][Cin]
                "cb": rnd(self.Cout, seed=3) * 0.5, "bw": rnd(self.Cout, seed=4, lo=0.5, hi=1.5),
                "bb": rnd(self.Cout, seed=5) * 0.2}

    def shapes(self):
        R = self.N * self.T
        return (R, self.Cin), (R, self.Cout)

    def hip(self, ops, P, x):
        C = self.Cout
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        nbt = torch.zeros((), dtype=torch.long, device="cuda")
        return ops.ConvBnActFn.apply(x, P["cw"], P["cb"], P["bw"], P["bb"], rm, rv, nbt, None, self.N, self.G, self.act, True)

    def ref(self, P, x):
        N, T, G = self.N, self.T, self.G
        xs = x.view(T, N, -1).permute(1, 2, 0)                 # frame-major rows t*N + n -> [N, Cin, T]
        per = N // G
        outs = []
        for g in range(G):                                    # one BatchNorm batch per group
            y = F.conv1d(xs[g * per:(g + 1) * per], P["cw"].permute(1, 2, 0), P["cb"], padding=2)
            z = F.batch_norm(y, None, None, P["bw"], P["bb"], training=True, eps=1e-5)
            outs.append(torch.tanh(z) if self.act == 2 else z)
        return torch.cat(outs, 0).permute(2, 0, 1).reshape(T * N, -1)

    def split(self, ops, mode):
        return {"cw"}

    compare = ("cw", "bw", "bb")                # (the pre-BatchNorm conv bias has a zero gradient: round-off only)


_LSTM_NAMES = ("w_ih", "w_hh", "b_ih", "b_hh")


class LstmCase:
    """LstmLayerFn: H = 64 bidirectional (the encoder's batched weight gradients), H = 512 / 1024 one direction with the
    persistent recurrence (bias gradients through row-group slabs) or the per-frame kernels."""

    def __init__(self, N, T, In, H, bidir, persistent):
        self.N, self.T, self.In, self.H, self.bidir, self.persistent = N, T, In, H, bidir, persistent
        self.name = f"lstm_h{H}{'_bidir' if bidir else ''}{'_pers' if persistent else '_frames'}"
        self.names = [n + s for s in ("", "_r")[:2 if bidir else 1] for n in _LSTM_NAMES]
        self.compare = tuple(self.names)

    def init(self):
        k = self.H ** -0.5
        shp = {"w_ih": (4 * self.H, self.In), "w_hh": (4 * self.H, self.H), "b_ih": (4 * self.H,), "b_hh": (4 * self.H,)}
        return {n: rnd(*shp[n.replace("_r", "")], seed=10 + i, lo=-k, hi=k) for i, n in enumerate(self.names)}

    def shapes(self):
        R = self.N * self.T
        return (R, self.In), (R, (2 if self.bidir else 1) * self.H)

    def hip(self, ops, P, x):
        ps = [P[n] for n in self.names] + ([None] * 4 if not self.bidir else [])
        return ops.LstmLayerFn.apply(x, self.T, self.N, *ps)

    def context(self, ops):
        return persistent_lstm(ops, self.persistent)          # read by the forward AND the backward launches

    def ref(self, P, x):
        return _lstm_ref(x, self.T, self.N, [[P[n + s] for n in _LSTM_NAMES] for s in ("", "_r")[:2 if self.bidir else 1]],
                         self.bidir)

    def split(self, ops, mode):
        from dvae_amd.derived import lstm_pack_modes
        out = {"w_ih", "w_hh"} | ({"w_ih_r", "w_hh_r"} if self.bidir else set())      # T = 8, N = 128: every one splits
        if self.persistent and not self.bidir:
            pers = ops.lstm_persistent_usable(self.N, self.H, lstm_pack_modes(mode, self.H)[1], 1, bwd=True)
            if mode == ops.MODE_F32X3:
                assert pers, "the default arithmetic has a persistent backward at this shape (N <= 128)"
            if pers:
                out |= {"b_ih", "b_hh"}                       # the row-group bias slabs, pending under both biases
        return out


class Stack2Case:
    N, T, In, H = 128, 8, 512, 1024
    name = "lstm_stack2"
    names = [n + s for s in ("1", "2") for n in _LSTM_NAMES]
    compare = tuple(names)

    def init(self):
        k = self.H ** -0.5
        shp = lambda n: {"w_ih": (4 * self.H, self.In if n.endswith("1") else self.H), "w_hh": (4 * self.H, self.H),
                         "b_ih": (4 * self.H,), "b_hh": (4 * self.H,)}[n[:-1]]
        return {n: rnd(*shp(n), seed=20 + i, lo=-k, hi=k) for i, n in enumerate(self.names)}

    def shapes(self):
        R = self.N * self.T
        return (R, self.In), (R, self.H)

    def hip(self, ops, P, x):
        assert ops.LstmStack2Fn.usable(self.T, self.H, 2, False)
        return ops.LstmStack2Fn.apply(x, self.T, self.N, *[P[n] for n in self.names])

    def ref(self, P, x):
        h = _lstm_ref(x, self.T, self.N, [[P[n + "1"] for n in _LSTM_NAMES]], False)
        return _lstm_ref(h, self.T, self.N, [[P[n + "2"] for n in _LSTM_NAMES]], False)

    def split(self, ops, mode):
        return {"w_ih1", "w_hh1", "w_ih2", "w_hh2"}


def _lstm_ref(x, T, N, dirs, bidir):
    """one nn.LSTM layer over frame-major rows [T*N, In] with the given (w_ih, w_hh, b_ih, b_hh) per direction"""
    outs = []
    for d, (wi, wh, bi, bh) in enumerate(dirs):
        H = wh.shape[1]
        h = x.new_zeros(N, H)
        c = x.new_zeros(N, H)
        xs = x.view(T, N, -1)
        hs = [None] * T
        for t in (reversed(range(T)) if d == 1 else range(T)):
            g = xs[t] @ wi.t() + bi + h @ wh.t() + bh
            i, f, gg, o = g.chunk(4, 1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            hs[t] = h
        outs.append(torch.stack(hs, 0))
    return torch.cat(outs, -1).reshape(T * N, -1)


CASES = [LinearCase(), ConvCase(1, 2), ConvCase(2, 0),                 # (ops.ACT_TANH, ops.ACT_NONE)
         LstmCase(128, 8, 128, 64, True, False),
         LstmCase(128, 8, 128, 512, False, True), LstmCase(128, 8, 128, 512, False, False),
         LstmCase(128, 8, 512, 1024, False, True), LstmCase(128, 8, 512, 1024, False, False),
         Stack2Case()]


def _inputs(case, uses, seed=0):
    xshape, yshape = case.shapes()
    xs = [rnd(*xshape, seed=100 + seed + i) for i in range(uses)]
    gs = [rnd(*yshape, seed=200 + seed + i) for i in range(uses)]
    return xs, gs


_REF = {}


def _reference(case, uses):
    """float64 CPU autograd of the same composition: {name: gradient}, [input gradients] (cached: mode independent)"""
    key = (case.name, uses)
    if key not in _REF:
        P = {n: v.double().requires_grad_() for n, v in case.init().items()}
        xs, gs = _inputs(case, uses)
        xs = [x.double().requires_grad_() for x in xs]
        outs = [case.ref(P, x) for x in xs]
        torch.autograd.backward(outs, [g.double() for g in gs])
        _REF[key] = ({n: p.grad for n, p in P.items()}, [x.grad for x in xs])
    return _REF[key]


def _owned(case):
    from dvae_amd.optim import FlatAdam
    P = {n: torch.nn.Parameter(v.cuda()) for n, v in case.init().items()}
    opt = FlatAdam(list(P.items()), lr=1e-3)
    return P, opt


def _pass(ops, case, P, xs, gs):
    """one graph that applies the op once per input, one backward pass"""
    xd = [x.cuda().requires_grad_() for x in xs]
    with (case.context(ops) if hasattr(case, "context") else contextlib.nullcontext()):
        outs = [case.hip(ops, P, x) for x in xd]
        torch.autograd.backward(outs, [g.cuda() for g in gs])
    return xd


@pytest.mark.parametrize("uses", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reused_owned_parameter_gradient_matches_fp64(ops, spy, case, uses):
    """`.grad` of an op applied `uses` times in one graph, read right after backward() (before any step), against float64;
    a second backward without zero_grad doubles it."""
    P, opt = _owned(case)
    xs, gs = _inputs(case, uses)
    ref, ref_dx = _reference(case, uses)
    xd = _pass(ops, case, P, xs, gs)
    assert not opt.__dict__.get("_slab_pending"), "k-split slabs still pending when backward() returned"
    seen = split_uses(spy, P)
    want = case.split(ops, ops.current_mode())
    assert all(seen.get(n, 0) >= uses for n in want), ("the deferred k-split path did not run for every use", want, seen)
    for n in case.compare:
        close(P[n].grad, ref[n], rel=GRAD_REL, name=f"{case.name}.{n} x{uses}")
    for i, x in enumerate(xd):
        close(x.grad, ref_dx[i], rel=GRAD_REL, name=f"{case.name} dx[{i}]")
    _pass(ops, case, P, xs, gs)                                # accumulates: no zero_grad in between
    assert not opt.__dict__.get("_slab_pending")
    for n in case.compare:
        close(P[n].grad, 2 * ref[n], rel=GRAD_REL, name=f"{case.name}.{n} x{uses}, second backward")


@pytest.mark.parametrize("uses", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_reused_owned_parameter_gradient_bf16_equals_sum_of_single_uses(spy, case, uses):
    """bf16 compute mode, the kernels as their own reference: the gradient of the pass that uses the op `uses` times equals
    the sum of the gradients of `uses` single-use passes to 1e-5 of its largest element."""
    import dvae_amd  # noqa: F401
    from dvae_amd import ops
    ops.set_compute_dtype("bf16")
    try:
        P, opt = _owned(case)
        xs, gs = _inputs(case, uses, seed=7)
        total = {n: torch.zeros(P[n].shape, dtype=torch.float64) for n in case.compare}
        for i in range(uses):
            opt.zero_grad()
            _pass(ops, case, P, xs[i:i + 1], gs[i:i + 1])
            for n in case.compare:
                total[n] += P[n].grad.detach().cpu().double()
        opt.zero_grad()
        del spy[:]
        _pass(ops, case, P, xs, gs)
        assert not opt.__dict__.get("_slab_pending")
        seen = split_uses(spy, P)
        want = case.split(ops, ops.MODE_BF16)
        assert all(seen.get(n, 0) >= uses for n in want), ("the deferred k-split path did not run for every use", want, seen)
        for n in case.compare:
            got = P[n].grad.detach().cpu().double()
            scale = max(1e-30, float(total[n].abs().max()))
            err = float((got - total[n]).abs().max())
            assert err <= 1e-5 * scale, f"{case.name}.{n} x{uses}: {err:.3e} vs scale {scale:.3e}"
    finally:
        ops.set_compute_dtype(ops.DEFAULT_COMPUTE_DTYPE)


# ---------------------------------------------------------------------------------------------------------- aborted backward
class _Boom(torch.autograd.Function):
    """identity whose backward raises on the host (no device work is involved)"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        raise RuntimeError("host-side failure inside backward")


def test_backward_that_raised_leaves_next_grad_complete(ops, spy):
    """A backward pass that raises skips autograd's final callbacks, with owned slabs pending.  After zero_grad, the next
    clean pass must sum its slabs when backward() returns — not only at the optimiser step.  (No activation: two stacked
    ReLUs put mask flips at round-off distance from zero into the float64 comparison.)"""
    from dvae_amd.optim import FlatAdam
    M, K = 2048, 512
    init = {"w1": rnd(K, K, seed=1) * 0.05, "b1": rnd(K, seed=2), "w2": rnd(K, K, seed=3) * 0.05, "b2": rnd(K, seed=4)}
    P = {n: torch.nn.Parameter(v.cuda()) for n, v in init.items()}
    opt = FlatAdam(list(P.items()), lr=1e-3)
    x, g = rnd(M, K, seed=5), rnd(M, K, seed=6)
    lin = lambda t, i: ops.LinearFn.apply(t, P[f"w{i}"], P[f"b{i}"], ops.ACT_NONE)
    xd = x.cuda().requires_grad_()
    y = lin(_Boom.apply(lin(xd, 1)), 2)
    with pytest.raises(RuntimeError, match="host-side failure"):
        y.backward(g.cuda())
    assert split_uses(spy, P).get("w2", 0) >= 1, "the aborted pass left no k-split slabs pending"
    opt.zero_grad()
    del spy[:]
    lin(lin(xd, 1), 2).backward(g.cuda())
    assert not opt.__dict__.get("_slab_pending"), "k-split slabs still pending when backward() returned"
    seen = split_uses(spy, P)
    assert seen.get("w1", 0) >= 1 and seen.get("w2", 0) >= 1, seen
    R = {n: v.double().requires_grad_() for n, v in init.items()}
    ref = lambda t, i: F.linear(t, R[f"w{i}"], R[f"b{i}"])
    ref(ref(x.double(), 1), 2).backward(g.double())
    for n in init:
        close(P[n].grad, R[n].grad, rel=GRAD_REL, name=n)


# ------------------------------------------------------------------------------------------------------------- model level
def test_reference_forward_on_the_public_api_matches_the_oracle(spy):
    """The reference's forward (disentangled_vae.py:250-279) written with the class-level API on a trainer's model: encode,
    decode and the postnet twice each, against the CPU oracle — losses, every parameter gradient (bounds of
    test_against_oracle_b8_t64_full_gradients), the BatchNorm buffers after their two updates — and against the same
    trainer's forward_full gradients."""
    from oracle.dvae_ref import RefTrainer, loss_gvae2
    from oracle.fill import fill_state_dict, synthetic_eps, synthetic_pair
    from test_hip_model import LOSS_RTOL, is_prebn_conv_bias, make, rel
    B, T = 8, 64
    w = make(B, T)
    w.optimizer.set_store_first(())            # enc_linear / dec_pre_linear2 get two contributions each
    m = w.model
    tr = RefTrainer(B, n_frames=T)
    tr.model.load_state_dict(fill_state_dict(tr.model.state_dict()))
    tr.model.train()
    x1, x2 = synthetic_pair(B, T, 77)
    eps = synthetic_eps(B, seed=5)
    outs_ref = tr.model(x1, x2, eps)
    l_ref = loss_gvae2(x1, x2, outs_ref, B)
    l_ref[0].backward()

    w.optimizer.zero_grad()
    x1c, x2c = x1.cuda(), x2.cuda()
    e_c1, e_c2, e_s = (e.cuda() for e in eps)
    s_mu1, s_lv1, c_mu1, c_lv1 = m.encode(x1c)
    s_mu2, s_lv2, c_mu2, c_lv2 = m.encode(x2c)
    z_c1 = e_c1 * torch.exp(0.5 * c_lv1) + c_mu1
    z_c2 = e_c2 * torch.exp(0.5 * c_lv2) + c_mu2
    s_mu = (s_mu1 + s_mu2.detach()) / 2
    s_lv = (s_lv1 + s_lv2.detach()) / 2
    z_s = e_s * torch.exp(0.5 * s_lv) + s_mu
    r1 = m.decode(torch.cat((z_s, z_c1), -1))
    r2 = m.decode(torch.cat((z_s, z_c2), -1))
    r1_hat = r1 + m.postnet(r1)
    r2_hat = r2 + m.postnet(r2)
    outs = (r1, r2, r1_hat, r2_hat, torch.cat((s_mu, c_mu1), -1), torch.cat((s_lv, c_lv1), -1),
            torch.cat((s_mu, c_mu2), -1), torch.cat((s_lv, c_lv2), -1), s_mu, s_lv)
    l = w.loss_functionGVAE2(x1c, x2c, *outs, train=True)
    l[0].backward()
    assert not w.optimizer.__dict__.get("_slab_pending"), "k-split slabs still pending when backward() returned"

    params = dict(m.named_parameters())
    seen = split_uses(spy, params)
    convs = [n for n in params if n.endswith("conv.weight") or (n.startswith("dec_modules.") and n.endswith(".0.weight"))]
    assert len(convs) == 11
    assert all(seen.get(n, 0) >= 2 for n in convs), ("conv weight gradients did not split on both uses", seen)
    print("owned k-split contributions per parameter:", seen)

    for i in range(8):
        assert rel(float(l[i].detach()), float(l_ref[i].detach())) <= LOSS_RTOL, (i, float(l[i]), float(l_ref[i]))
    ref_params = dict(tr.model.named_parameters())

    def grad_errors(grads, against):
        bad = []
        for n in params:
            gr = against[n].double()
            err = float((grads[n] - gr).norm())
            if is_prebn_conv_bias(n):
                if err > 0.2:
                    bad.append((n, err))
            elif err > 5e-3 * float(gr.norm()):
                bad.append((n, err, float(gr.norm())))
        return bad

    api = {n: m.reference_layout(n, p.grad).detach().cpu().double() for n, p in params.items()}
    bad = grad_errors(api, {n: p.grad for n, p in ref_params.items()})
    assert not bad, bad
    sd, sd_ref = m.state_dict(), tr.model.state_dict()
    for k, v in sd_ref.items():
        if "running_" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=2e-4, atol=1e-5, err_msg=k)
        elif k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 2, k

    w.optimizer.zero_grad()
    m.eps_override = eps
    outs_full = m(x1c, x2c)
    w.loss_functionGVAE2(x1c, x2c, *outs_full, train=True)[0].backward()
    full = {n: m.reference_layout(n, p.grad).detach().cpu() for n, p in params.items()}
    bad = grad_errors(api, full)
    assert not bad, bad
