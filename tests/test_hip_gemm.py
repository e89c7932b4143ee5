"""The contraction kernels (csrc/gemm.hip, csrc/gemm256.hip: every kernel behind dvae_gemm_f32, _batched, _slabs,
_batched_slabs and the dvae_conv5_* entry points) held to an EXACT product, element by element, through the C ABI.

`gemm_ref.CASES` holds the smallest shape that reaches each kernel and path; every case runs the input classes that apply to
it (tests/gemm_ref.py): E1 (selection), E2 (small integers), E3 (two-term integers) must come back bit for bit — one lost,
doubled or mis-addressed term fails at tolerance zero at the element where it happened — and R (full significands, a row and
a column block 2^12 apart, a zero row block) within 2 rho_max S_ij at EVERY element and 2 rho_rms in the RMS, rho measured on a
CPU restatement of the arithmetic, never on the device.  Every launch of a case runs under the launch profiler and the tag it
recorded must equal the restated dispatch (kernel, A_KC, B_KC, NTW, BK, WG, MODE, BNS, A16, B16, tap mode): a retuned threshold
that moves a case to another kernel fails here instead of passing vacuously.  Around every result: the padding columns of
ldc > N, the guard elements in front of and behind C, the slabs behind the used ones and C itself under a split slab launch
keep their poison.  The worst error / bound per kernel family and class is printed at the module's end."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import DEV, L, ok, st      # first: it puts the repository root on sys.path
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib, ops  # noqa: E402
import gemm_ref as G  # noqa: E402

F = np.float32
POISON = -1.2345678e30                      # what untouched memory holds
GUARD = 136                                 # guard elements on either side of C: at least 256 bytes in fp32 and bf16, and
                                            # 8 elements behind a multiple of 256 bytes, so C keeps the offset it had
WORST = {}                                  # (kernel family, class) -> worst error / bound (exact classes: 0 = every bit held)
RHO = {}
T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    ops.prof_enable(0)
    fams = sorted({f for f, _ in WORST})
    cols = ["E1", "E2", "E3", "R max", "R rms"]
    print("\nworst error / bound per kernel family (E1 - E3: 0 = every element bit-exact):")
    print("| kernels | " + " | ".join(cols) + " |")
    for f in fams:
        print(f"| {f} | " + " | ".join(f"{WORST[(f, c)]:.3f}" if (f, c) in WORST else "" for c in cols) + " |")
    print(f"{len(G.CASES)} cases, {time.time() - T0:.1f} s")


def dev(x, bf=False):
    t = torch.from_numpy(np.ascontiguousarray(x, F)).to(DEV)
    return t.bfloat16() if bf else t


def op_a(a, kc, bf):
    """logical a [M, K] as the device stores it: [M][K] (k-contiguous) or [K][M]"""
    return dev(a if kc else a.T, bf)


def op_b(b, kc, bf):
    """logical b [K, N]: [N][K] (k-contiguous) or [K][N]"""
    return dev(b.T if kc else b, bf)


class CBuf:
    """C [M, ldc] inside a poisoned buffer: GUARD elements in front (+ c_off to misalign), the padding columns, GUARD behind."""

    def __init__(self, M, N, ldc, c_off=0, base=None, bf=False, nmat=1):
        self.M, self.N, self.ldc, self.nmat, self.bf = M, N, ldc, nmat, bf
        self.off = GUARD + c_off
        host = np.full(self.off + nmat * M * ldc + GUARD, POISON, F)
        if base is not None:
            v = host[self.off:self.off + nmat * M * ldc].reshape(nmat, M, ldc)
            for i in range(nmat):
                v[i, :, :N] = base[i]
        self.t = dev(host, bf)
        self.before = self.t.clone()

    @property
    def ptr(self):
        return self.t.data_ptr() + self.t.element_size() * self.off

    def n_el(self):
        return self.nmat * self.M * self.ldc

    def read(self):
        """([nmat] results [M, N] fp32, failures of the poison around them)"""
        torch.cuda.synchronize()
        h = self.t.float().cpu().numpy()
        b = self.before.float().cpu().numpy()
        v = h[self.off:self.off + self.n_el()].reshape(self.nmat, self.M, self.ldc)
        fails = []
        keep = np.ones(h.shape, bool)
        kv = keep[self.off:self.off + self.n_el()].reshape(self.nmat, self.M, self.ldc)
        kv[:, :, :self.N] = False
        if not np.array_equal(h[keep].view(np.uint32), b[keep].view(np.uint32)):
            fails.append(f"{int((h[keep] != b[keep]).sum())} elements outside C [M, N] (guards, padding columns of ldc) were written")
        return [np.ascontiguousarray(v[i, :, :self.N]) for i in range(self.nmat)], fails

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.t.view(torch.int16 if self.bf else torch.int32), self.before.view(torch.int16 if self.bf else torch.int32))


def pad4(n):
    return (n + 3) // 4 * 4


def fold(cbufs, slab, stride, n, n_el, accumulate, use_fold):
    """C (+)= the n slabs of each result, in the fixed order, by dvae_slab_sum or (Case.use_fold; it only accumulates)
    dvae_slab_fold"""
    assert accumulate or not use_fold
    if use_fold:
        descs = []
        for b, cb in enumerate(cbufs):
            d = _lib.SlabDesc()
            d.c, d.slab, d.slab_stride, d.n, d.nslab = cb.ptr, slab.data_ptr() + 4 * b * n * stride, stride, n_el, n
            descs.append(d)
        ok(L().dvae_slab_fold((_lib.SlabDesc * len(descs))(*descs), len(descs), st()), "dvae_slab_fold")
    else:
        for b, cb in enumerate(cbufs):
            ok(L().dvae_slab_sum(cb.ptr, slab.data_ptr() + 4 * b * n * stride, stride, n, n_el, 0, int(accumulate), st()),
               "dvae_slab_sum")


def slabs_check(slab, stride, used, cap_total):
    """the slabs behind the used ones keep their poison"""
    torch.cuda.synchronize()
    tail = slab[used * stride:]
    return [] if bool((tail == POISON).all()) else [f"slabs behind the {used} used ones (of {cap_total}) were written"]


def run(c, d, inp):
    """One launch (plus the fold of its slabs) of case c on inputs inp -> (outputs, failures, extra)."""
    mode = G.MODES[c.mode] | (G.A_BF16 if c.a16 else 0) | (G.B_BF16 if c.b16 else 0) | (G.C_BF16 if c.c16 else 0)
    M, N, K = c.M, c.N, c.K
    bias = None if inp.bias is None else dev(inp.bias)
    bp = None if bias is None else bias.data_ptr()
    fails, extra = [], {}
    lib = L()
    if not G.is_conv(c):
        As = inp.a if c.batch > 1 else [inp.a]
        Bs = inp.b if c.batch > 1 else [inp.b]
        dA = [op_a(a, c.a_kc, c.a16) for a in As]
        dB = [op_b(b, c.b_kc, c.b16) for b in Bs]
        if c.shared_b:
            dB = [dB[0]] * c.batch
        lda, ldb, ldc = (K if c.a_kc else M), (K if c.b_kc else N), N + c.ldc_pad
        cbs = [CBuf(M, N, ldc, c.c_off, None if inp.base is None else [inp.base[i]], c.c16) for i in range(c.batch)]
        arr = lambda xs: (C.c_void_p * len(xs))(*xs)
        pa, pb, pc = [t.data_ptr() for t in dA], [t.data_ptr() for t in dB], [cb.ptr for cb in cbs]
        if c.entry == "gemm":
            ok(lib.dvae_gemm_f32(pa[0], pb[0], pc[0], bp, M, N, K, lda, ldb, ldc, int(c.a_kc), int(c.b_kc), c.act, c.epi,
                                 c.split, mode, st()), "dvae_gemm_f32")
        elif c.entry == "batched":
            ok(lib.dvae_gemm_f32_batched(arr(pa), arr(pb), arr(pc), c.batch, M, N, K, lda, ldb, ldc, int(c.a_kc), int(c.b_kc),
                                         c.epi, c.split, mode, st()), "dvae_gemm_f32_batched")
        else:
            stride = pad4(M * ldc)
            cap = c.slab_cap
            slab = torch.full(((max(cap, 1) + 2) * stride,), POISON, device=DEV)
            if c.entry == "slabs":
                n = lib.dvae_gemm_f32_slabs(pa[0], pb[0], pc[0], slab.data_ptr(), stride, cap, bp, M, N, K, lda, ldb, ldc,
                                            int(c.a_kc), int(c.b_kc), c.epi, c.split, mode, st())
            else:
                n = lib.dvae_gemm_f32_batched_slabs(arr(pa), arr(pb), arr(pc), c.batch, slab.data_ptr(), stride, cap, M, N, K,
                                                    lda, ldb, ldc, int(c.a_kc), int(c.b_kc), c.epi, c.split, mode, st())
            assert n == d["split_k"], f"{n} k-splits launched, the restated dispatch says {d['split_k']}"
            fails += slabs_check(slab, stride, n * c.batch if n > 1 else 0, cap)
            if n > 1:
                if not all(cb.untouched() for cb in cbs):
                    fails.append("a split slab launch wrote C")
                fold(cbs, slab, stride, n, M * ldc, c.epi == G.EPI_ACCUM, use_fold=c.use_fold)
        outs = []
        for cb in cbs:
            o, f = cb.read()
            outs += o
            fails += f
        return outs, fails, extra
    # ---- the convs.  Case dims: forward / data gradient M = R rows, N = output columns, K = input columns of the product;
    # weight gradient M = Cout, N = Cin, K = R
    if G.is_wgrad(c):
        Cout, Cin, R = M, N, K
        dY, X = dev(inp.a.T), dev(inp.b)
        cb = CBuf(Cout, Cin, Cin, 0, inp.base, nmat=5)
        if c.entry == "conv_wgrad":
            ok(lib.dvae_conv5_wgrad(dY.data_ptr(), X.data_ptr(), cb.ptr, R, c.nseg, Cin, Cout, c.split, mode, st()), "dvae_conv5_wgrad")
        else:
            stride = pad4(5 * Cout * Cin)
            slab = torch.full(((c.slab_cap + 2) * stride,), POISON, device=DEV)
            n = lib.dvae_conv5_wgrad_slabs(dY.data_ptr(), X.data_ptr(), cb.ptr, slab.data_ptr(), stride, c.slab_cap, R, c.nseg, Cin,
                                           Cout, c.epi, c.split, mode, st())
            assert n == d["split_k"], f"{n} k-splits launched, the restated dispatch says {d['split_k']}"
            fails += slabs_check(slab, stride, n if n > 1 else 0, c.slab_cap)
            if n > 1:
                if not cb.untouched():
                    fails.append("a split slab launch wrote C")
                fold([cb], slab, stride, n, 5 * Cout * Cin, c.epi == G.EPI_ACCUM, use_fold=c.use_fold)
        outs, f = cb.read()
        return outs, fails + f, extra
    R, Nout, Kin = M, N, K
    X = dev(inp.a, c.a16)
    Wp = dev(inp.b.reshape(5, Kin, Nout).transpose(0, 2, 1), c.b16)      # [tap][out column][k]
    cb = CBuf(R, Nout, Nout, 0, None)
    if c.entry == "conv_fwd":
        ok(lib.dvae_conv5_fwd(X.data_ptr(), Wp.data_ptr(), bp, cb.ptr, R, c.nseg, Kin, Nout, mode, st()), "dvae_conv5_fwd")
    elif c.entry == "conv_dgrad":
        ok(lib.dvae_conv5_dgrad_t(X.data_ptr(), Wp.data_ptr(), cb.ptr, R, c.nseg, Nout, Kin, mode, st()), "dvae_conv5_dgrad_t")
    elif c.entry == "conv_fwd_stats":
        nbytes = int(lib.dvae_bn_ws_bytes(R, Nout, c.G))
        ws = torch.full((nbytes // 8 + 1,), float("nan"), device=DEV, dtype=torch.float64)
        ok(lib.dvae_conv5_fwd_stats(X.data_ptr(), Wp.data_ptr(), bp, cb.ptr, R, c.nseg, Kin, Nout, mode, c.G, ws.data_ptr(), st()),
           "dvae_conv5_fwd_stats")
        extra["ws"] = ws
    else:
        stride = pad4(R * Nout)
        slab = torch.full(((c.slab_cap + 2) * stride,), POISON, device=DEV)
        if c.entry == "conv_fwd_slabs":
            n = lib.dvae_conv5_fwd_slabs(X.data_ptr(), Wp.data_ptr(), bp, cb.ptr, slab.data_ptr(), stride, c.slab_cap, R, c.nseg, Kin,
                                         Nout, mode, st())
        else:
            n = lib.dvae_conv5_dgrad_t_slabs(X.data_ptr(), Wp.data_ptr(), cb.ptr, slab.data_ptr(), stride, c.slab_cap, R, c.nseg,
                                             Nout, Kin, mode, st())
        assert n == d["split_k"], f"{n} k-splits launched, the restated dispatch says {d['split_k']}"
        fails += slabs_check(slab, stride, n if n > 1 else 0, c.slab_cap)
        if n > 1:
            if not cb.untouched():
                fails.append("a split slab launch wrote C")
            fold([cb], slab, stride, n, R * Nout, False, use_fold=False)
    outs, f = cb.read()
    return outs, fails + f, extra


def stats_check(c, y, ws):
    """dvae_conv5_fwd_stats under E2: the per-chunk fp64 sums and sums of squares are exact integers — equal to the
    standalone statistics of the (exactly checked) Y, group by group."""
    R, Nn = y.shape
    assert 64 * float(np.abs(y).max()) ** 2 < 1 << 24, "the squares of this case do not sum exactly in fp32"
    nch = (R + 63) // 64
    got = ws[:nch * c.G * Nn * 2].cpu().numpy().reshape(nch, c.G, Nn, 2)
    y64 = np.zeros((nch * 64, Nn))
    y64[:R] = y
    grp = np.zeros(nch * 64, int)
    grp[:R] = (np.arange(R) % c.nseg) // (c.nseg // c.G)
    want = np.zeros_like(got)
    for g in range(c.G):
        sel = (y64 * (grp == g)[:, None]).reshape(nch, 64, Nn)
        want[:, g, :, 0] = sel.sum(1)
        want[:, g, :, 1] = (sel * sel).sum(1)
    return G.exact_check(got, want, "BatchNorm partial statistics [chunk, group, column, (sum, sum of squares)]")


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_case(c):
    d = G.expected_kernel(c)
    assert d is not None
    fails = []
    if c.deterministic:
        ok(L().dvae_set_deterministic(1), "dvae_set_deterministic")
    ops.prof_enable(1)
    try:
        for inp in G.iter_inputs(c, d):
            outs, f, extra = run(c, d, inp)
            fails += [f"{inp.cls}: {x}" for x in f]
            fails += G.judge(c, d, inp, outs, RHO, WORST)
            if "ws" in extra and inp.cls == "E2":
                fails += stats_check(c, outs[0], extra["ws"])
        torch.cuda.synchronize()
        tags = [t["tag"] for t in ops.prof_collect_tags()]
        ops.prof_collect()
    finally:
        ops.prof_enable(0)
        if c.deterministic:
            ok(L().dvae_set_deterministic(int(ops.deterministic())), "dvae_set_deterministic")
    want = {k: d[k] for k in G.TAG_FIELDS}
    assert tags and all(G.decode_tag(t) == want for t in tags), \
        f"reached {[G.decode_tag(t) for t in tags]}, the restated dispatch (and the case) name {want}"
    for k, v in (c.reach or {}).items():
        assert d[k] == v
    assert not fails, "\n".join(fails[:12])


def test_deterministic_flag_takes_the_unsplit_path_with_identical_bits():
    """narrow_conv_split cuts the 80-column conv along k and accumulates atomically; dvae_set_deterministic(1) runs it
    unsplit.  Under E2 both are the exact product: identical bits."""
    c1, c2 = G.CASE_BY_NAME["conv-fwd-narrow-split"], G.CASE_BY_NAME["conv-fwd-narrow-deterministic"]
    inp = G.make_inputs(c1, "E2")
    res = []
    for c in (c1, c2):
        d = G.expected_kernel(c)
        try:
            if c.deterministic:
                ok(L().dvae_set_deterministic(1), "dvae_set_deterministic")
            outs, f, _ = run(c, d, inp)
        finally:
            ok(L().dvae_set_deterministic(int(ops.deterministic())), "dvae_set_deterministic")
        assert not f, f
        res.append(outs[0])
    assert G.expected_kernel(c1)["split_k"] == 2 and G.expected_kernel(c2)["split_k"] == 1
    assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
