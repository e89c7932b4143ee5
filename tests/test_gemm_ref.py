"""tests/gemm_ref.py proved on the CPU, before any GPU number is read: the reference against torch in float64 (matmul, F.conv1d
forward and both gradients through autograd), the exactness of the classes E1 - E3 in every summation order, the workgroup ->
tile map as a bijection, the restated dispatch over `CASES` (every case reaches the kernel it names, every instantiation of
the product build is reached), the bounds of class R on both restated orders of each arithmetic, and fifteen mutations of the
restated arithmetic, each of which the classes named in `MUTANTS` must flag at the smallest case that can show it.  `CAUGHT`
records which class caught which mutant (DESIGN.md section 5 lists it)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G  # noqa: E402

F, F64 = np.float32, np.float64
CAUGHT = {}


# ----------------------------------------------------------------------------------------------------- the reference
def test_reference_equals_torch_float64_matmul():
    rs = np.random.default_rng(1)
    a, b = rs.standard_normal((37, 53)), rs.standard_normal((53, 29))
    ref = (torch.from_numpy(a) @ torch.from_numpy(b)).numpy()
    assert np.abs(G.mm_exact(a, b) - ref).max() <= 1e-12 * np.abs(ref).max()
    c = G.Case(name="x", M=37, N=29, K=53, mode="fp32", bias=True, act=G.ACT_RELU, epi=G.EPI_ACCUM)
    bias, base = rs.standard_normal(29), rs.standard_normal((37, 29))
    u, z, S = G.r_reference(c, a.astype(F), b.astype(F), bias.astype(F), base.astype(F))
    t = lambda x: torch.from_numpy(np.asarray(x, F).astype(F64))
    zt = torch.relu(t(a) @ t(b) + t(bias)) + t(base)
    assert np.abs(z - zt.numpy()).max() <= 1e-12 * np.abs(z).max()
    assert np.abs(S - (t(a).abs() @ t(b).abs() + t(bias).abs() + t(base).abs()).numpy()).max() <= 1e-12 * S.max()


@pytest.mark.parametrize("nseg,T", [(1, 1), (2, 2), (5, 3), (2, 5), (3, 9)])
def test_conv_products_equal_conv1d_and_its_gradients(nseg, T):
    """`products` of the three conv entry points against F.conv1d(padding=2) in float64 and autograd."""
    Cin, Cout, R = 12, 8, nseg * T
    rs = np.random.default_rng(nseg * 10 + T)
    x = torch.from_numpy(rs.standard_normal((nseg, Cin, T))).requires_grad_()
    w = torch.from_numpy(rs.standard_normal((Cout, Cin, 5))).requires_grad_()
    gy = torch.from_numpy(rs.standard_normal((nseg, Cout, T)))
    y = Fn.conv1d(x, w, None, padding=2)
    y.backward(gy)
    fr = lambda t: t.detach().permute(2, 0, 1).reshape(R, -1).numpy()      # [n, C, T] -> frame-major rows [T n, C]
    X, dY = fr(x), fr(gy)
    wn = w.detach().numpy()
    close = lambda got, ref: np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    # forward: b = the taps side by side, b[tap Cin + ci, co] = W[co, ci, tap]
    c = G.Case(name="f", entry="conv_fwd", M=R, N=Cout, K=Cin, nseg=nseg)
    (a_eff, b_eff), = G.products(c, X, wn.transpose(2, 1, 0).reshape(5 * Cin, Cout))
    assert close(G.mm_exact(a_eff, b_eff), fr(y))
    # data gradient: b[tap Cout + co, ci] = W[co, ci, tap], rows shifted the other way
    c = G.Case(name="d", entry="conv_dgrad", M=R, N=Cin, K=Cout, nseg=nseg)
    (a_eff, b_eff), = G.products(c, dY, wn.transpose(2, 0, 1).reshape(5 * Cout, Cin))
    assert close(G.mm_exact(a_eff, b_eff), fr(x.grad))
    # weight gradient: one product per tap, dWp[tap][co][ci]
    c = G.Case(name="w", entry="conv_wgrad", M=Cout, N=Cin, K=R, nseg=nseg)
    for tap, (a_eff, b_eff) in enumerate(G.products(c, dY.T.copy(), X)):
        assert close(G.mm_exact(a_eff, b_eff), w.grad.numpy()[:, :, tap])


# ----------------------------------------------------------------------------------------------------- the classes
def _orders(K, splits):
    """k orders: forward, reverse, and tile-blocked (tiles of 16, 32, 64; each split's partial formed first)."""
    yield "fwd", [list(range(K))]
    yield "rev", [list(range(K - 1, -1, -1))]
    for bk in (16, 32, 64):
        for sk in splits:
            kps = -(-(-(-K // sk)) // bk) * bk
            yield f"bk{bk}-sk{sk}", [list(range(t, min(t + bk, k0 + kps, K))) for k0 in range(0, K, kps)
                                      for t in range(k0, min(k0 + kps, K), bk)]


def _fp32_ok(x):
    x = np.asarray(x, F64)
    return bool(np.all(x.astype(F).astype(F64) == x))


def _prefixes_representable(terms, groups, extra):
    """Every prefix of the accumulation (term planes inside a k step in both directions, group partials formed first, then
    added; the bias and the base last or first) is an fp32 number."""
    for rev in (False, True):
        tt = terms[::-1] if rev else terms
        total = np.zeros_like(np.asarray(tt[0][0], F64)[:, :1] * np.asarray(tt[0][1], F64)[:1])
        for first in (False, True):
            total = total * 0 + (extra if first else 0.0)
            for grp in groups:
                part = total * 0
                for k in grp:
                    for ta, tb in tt:
                        part = part + np.asarray(ta, F64)[:, k:k + 1] * np.asarray(tb, F64)[k]
                        if not _fp32_ok(part) or not _fp32_ok(total + part):
                            return False
                total = total + part
            if not _fp32_ok(total + (0.0 if first else extra)):
                return False
    return True


SPLITS_USED = sorted({G.expected_kernel(c)["split_k"] for c in G.CASES if G.expected_kernel(c)["split_k"] <= 8})


@pytest.mark.parametrize("cls,mode", [(c, m) for c in ("E1", "E2", "E3") for m in ("fp32", "fp32x3", "bf16")
                                      if (c, m) != ("E3", "bf16")])      # E3 needs two bf16 terms per operand
def test_classes_are_exact_in_every_order(cls, mode):
    M, N, K = 9, 11, 84
    m = G.MODES[mode]
    for role in (("A", "B") if cls != "E2" else (None,)):
        for r in ((0, 5, K - 3) if cls != "E2" else (0,)):
            if cls == "E1":
                a, b = G.e1("t", M, N, K, role, r)
                extra = 0.0
            elif cls == "E3":
                a, b = G.e3("t", M, N, K, role, r)
                extra = 0.0
            else:
                a, b, bias, base = G.e2("t", M, N, K, True, True)
                extra = bias.astype(F64)[None] + base.astype(F64)
            terms = G.terms_of(a, b, m)
            if m == G.MODE_F32X3:
                pa, pb = G.split3(a), G.split3(b)
                assert np.array_equal(pa[0].astype(F64) + pa[1] + pa[2], a.astype(F64))
                assert np.array_equal(pb[0].astype(F64) + pb[1] + pb[2], b.astype(F64))
                if cls == "E1":       # every split term of the arbitrary operand is a normal number
                    dense = pa if role == "B" else pb
                    assert all(np.all((np.abs(p) >= 2.0 ** -126) | (p == 0)) for p in dense)
            for name, groups in _orders(K, SPLITS_USED):
                assert _prefixes_representable(terms, groups, extra), (cls, mode, role, r, name)
            # ... and both restated orders return the exact value
            c = G.Case(name="t", M=M, N=N, K=K, mode=mode, bias=cls == "E2", epi=G.EPI_ACCUM if cls == "E2" else G.EPI_STORE)
            bias_, base_ = (bias, base) if cls == "E2" else (None, None)
            want = G.expected_exact(c, a, b, bias_, base_)
            for order in ("seq", "tile"):
                for kps in (None, 32):
                    assert not G.exact_check(G.restate(a, b, m, order, bias_, base_, kps), want)


def test_e1_offsets_visit_what_the_module_says():
    """Every case (index arithmetic only): while K <= 6 min(M, N) the offsets select EVERY k; else the first and the last k and
    both sides of the first four split boundaries.  The conv forward / data gradient: every tap, one nonzero per column."""
    for c in G.CASES:
        d = G.expected_kernel(c)
        if G.is_conv(c) and not G.is_wgrad(c):
            continue
        M, N, K = G.logical_dims(c)
        n, kps = min(M, N), d["k_per_split"]
        seen = set()
        for r in G.offsets_of(c, "E1", d):
            seen.update(int(k) for k in (np.arange(n) + r) % K)
        if -(-K // n) <= 6:
            assert len(seen) == K, c.name
        else:
            assert 0 in seen and K - 1 in seen, c.name
            for kb in list(range(kps, K, kps))[:4]:
                assert kb - 1 in seen and kb in seen, (c.name, kb)
    c = G.CASE_BY_NAME["conv-fwd-n2-t3"]
    for r in G.offsets_of(c, "E1", G.expected_kernel(c)):
        inp = G.make_inputs(c, "E1", "B", r)
        taps = {int(k) // c.K for k in np.argwhere(inp.b != 0)[:, 0]}
        assert taps == set(range(5)) and np.all((inp.b != 0).sum(0) == 1)


def test_e2_and_e3_stay_below_2_to_24_in_every_case():
    for c in G.CASES:
        K = G.logical_dims(c)[2]
        if "E2" in c.classes:
            assert K * 225 + 1000 + 100000 < 1 << 24, c.name
        if "E3" in c.classes:
            assert c.mode != "bf16", c.name
    # E3 through the split: sum over <= 8 nonzeros of (|x1| + |x2|)(|y1| + |y2|) stays below 2^24 too
    v = np.arange(1, 1024, 2).astype(F)
    p = G.split3(v)
    assert np.all(p[2] == 0) and np.any(p[1] != 0)
    assert 8 * float((np.abs(p[0]) + np.abs(p[1])).max()) ** 2 < 1 << 24


# ----------------------------------------------------------------------------------------------------- the tile map
def test_tile_map_is_a_bijection():
    """gemm_tile_of restated, with the map_gm / map_gn / map_nstr the restated host side computes, and with the map off."""
    for tall in (False, True):
        for tm in range(1, 65):
            for tn in range(1, 41):
                # a launch with exactly tm x tn tiles of its kernel: 128 x 64 (narrow, fp32) or 256 x 128 (fp32x3 tall)
                if tall:
                    d = G.launch_gemm(256 * tm, 128 * tn, 128, True, True, G.MODE_F32X3)
                    if d["kernel"] != "x3_tall":
                        continue
                else:
                    d = G.launch_gemm(128 * tm, 64 * tn, 48, True, True, G.MODE_F32)
                    if not d["narrow"]:
                        d = G.launch_gemm(128 * tm, 128 * tn, 48, True, True, G.MODE_F32)
                assert (d["tiles_m"], d["tiles_n"]) == (tm, tn) and d["xcd_map"] == int(tm % 8 == 0)
                assert d["map_gn"] * d["map_nstr"] == tn and (tm // 8) % d["map_gm"] == 0 if d["xcd_map"] else True
                for off in ((False, True) if d["xcd_map"] else (True,)):
                    dd = dict(d, xcd_map=0) if off else d
                    tiles = {G.tile_of(bid, dd) for bid in range(tm * tn)}
                    assert tiles == {(i, j) for i in range(tm) for j in range(tn)}, (tm, tn, off)
    for tn, gn in ((1, 1), (3, 3), (7, 7), (9, 3), (11, 1)):
        for tm in (8, 16, 24):
            d = G.expected_kernel(G.CASE_BY_NAME[f"xcd-{tm}x{tn}"])
            assert d["map_gn"] == gn and d["xcd_map"] == 1
            assert d["map_gm"] > 1 or tm == 8
    # with xcd_map, XCD x (blockIdx.x & 7) owns the contiguous m-tiles [x per, (x + 1) per)
    d = G.expected_kernel(G.CASE_BY_NAME["xcd-24x9"])
    for bid in range(24 * 9):
        assert G.tile_of(bid, d)[0] // 3 == bid & 7


# ----------------------------------------------------------------------------------------------------- the dispatch
def test_every_case_reaches_the_kernel_it_names():
    reached = set()
    for c in G.CASES:
        d = G.expected_kernel(c)
        assert d is not None, f"{c.name}: the ABI rejects this launch"
        for k, v in (c.reach or {}).items():
            assert d[k] == v, f"{c.name}: {k} = {d[k]}, the case names {v}"
        assert G.decode_tag(d["tag"]) == {k: d[k] for k in G.TAG_FIELDS}
        reached.add(G.instantiation(d))
    every = G.all_instantiations()
    assert reached <= every, sorted(reached - every)
    missing = every - reached
    assert not missing and not G.UNREACHED, f"instantiations no case reaches: {sorted(missing)}"


def test_dispatch_restatement_on_known_launches():
    """Launches whose kernel the existing GPU tests and DESIGN.md state: the tall tile from 192 tiles and 8 k-steps on, the
    K % 16 neighbour falling back, the 16-wave fp32 tile, the 256 x 256 bf16 tile, the narrow conv split."""
    L = G.launch_gemm
    assert L(16384, 512, 1024, True, True, G.MODE_F32X3)["kernel"] == "x3_tall"
    assert L(6144, 1024, 128, True, True, G.MODE_F32X3)["kernel"] == "x3_tall"
    assert L(6144 - 256, 1024, 128, True, True, G.MODE_F32X3)["kernel"] == "f32"
    assert L(6144, 1024, 112, True, True, G.MODE_F32X3)["kernel"] == "f32"
    assert L(6144, 1024, 136, True, True, G.MODE_F32X3)["kernel"] == "f32"
    assert L(8192, 4096, 64, True, True, G.MODE_F32)["WG"] == 4 and L(8192, 4096, 48, True, True, G.MODE_F32)["WG"] == 2
    assert L(16384, 512, 1024, True, True, G.MODE_BF16, a16=True, b16=True)["kernel"] == "bf16_tall"
    assert L(4096, 3584, 512, True, True, G.MODE_BF16, a16=True, b16=True)["kernel"] == "bf16_256"
    assert L(4096, 3584 - 256, 512, True, True, G.MODE_BF16, a16=True, b16=True)["kernel"] == "bf16_tall"
    assert L(4096, 3584, 512, True, False, G.MODE_BF16, a16=True, b16=True)["kernel"] == "bf16_tall"
    assert L(130, 32, 36, True, True, G.MODE_F32)["NTW"] == 2 and L(200, 72, 80, True, True, G.MODE_F32)["NTW"] == 1
    assert L(128, 128, 48, True, True, G.MODE_F32)["BK"] == 16 and L(128, 128, 64, True, True, G.MODE_F32)["BK"] == 32
    assert L(8, 2048, 6, False, False, G.MODE_F32) is not None and L(8, 2048, 6, True, False, G.MODE_F32) is None
    assert L(130, 72, 80, False, True, G.MODE_F32) is None and L(130, 72, 80, True, True, G.MODE_F32, split_k=2) is None
    assert G.narrow_conv_split(16384, 80, 512, G.MODE_F32X3, False, False, 0) == (4, True)
    assert G.narrow_conv_split(16384, 80, 512, G.MODE_F32X3, True, False, 0) is None
    assert G.narrow_conv_split(16384, 80, 512, G.MODE_F32, False, False, 0) is None
    assert G.narrow_conv_split(95 * 256, 80, 160, G.MODE_F32X3, False, False, 0) is None
    assert G.narrow_conv_split(95 * 256 + 1, 80, 160, G.MODE_F32X3, False, True, 4) == (2, False)


# ----------------------------------------------------------------------------------------------------- the bounds of R
def model(c, inp, order="tile", mut=None):
    """A case's outputs as the restated arithmetic gives them (the stand-in for the device on the CPU), with a mutation."""
    mut = mut or {}
    d = G.expected_kernel(c)
    mode = G.MODES[c.mode]
    a_in, b_in = inp.a, inp.b
    if mut.get("batched_b0"):
        b_in = [b_in[0]] * len(b_in)
    if mut.get("wgrad_sign"):
        prods = [(a_in, G.shift_rows(b_in, -(t - 2) * G.tap_shift(c))) for t in range(G.TAPS)]
    elif mut.get("no_padding"):      # the rows before the sequence start are read from the sequence's other end
        x = a_in
        cat = np.concatenate([np.where((np.arange(x.shape[0]) + (t - 2) * G.tap_shift(c) < 0)[:, None],
                                       np.roll(x, -(t - 2) * G.tap_shift(c), axis=0),
                                       G.shift_rows(x, (t - 2) * G.tap_shift(c))) for t in range(G.TAPS)], axis=1)
        prods = [(cat, b_in)]
    else:
        prods = G.products(c, a_in, b_in)
    kps = d["k_per_split"] * (G.TAPS if G.is_conv(c) and not G.is_wgrad(c) else 1)
    outs = []
    for i, (a, b) in enumerate(prods):
        base = None if inp.base is None else inp.base[i]
        u = G.restate(a, b, mode, order, inp.bias, None if c.act != G.ACT_NONE else base, kps, mut)
        if c.act != G.ACT_NONE:
            u = np.asarray(G.act_apply(u.astype(F64), c.act), F)
        if c.c16:
            u = G.bf16(u)
        if mut.get("tile_map"):          # tile (0, 0) never written (it keeps what the buffer held), tile (1, 0) written twice
            u = u.copy()
            u[:min(d["bm"], u.shape[0]), :min(d["bn"], u.shape[1])] = -7.0
        outs.append(u)
    return outs


# every arithmetic x every epilogue (store, bias + ReLU / tanh, ACCUM with and without 16-byte stores, atomic splits, ldc
# padding, unaligned C, the bf16 store), the slab folds, a batched launch and the three conv products, by name
R_CASES = [c for c in G.CASES if c.name.startswith("epi-")] + [G.CASE_BY_NAME[n] for n in (
    "slabs-split4", "slabs-clamp", "slabs-bf16", "batched3-accum", "batched2-slabs", "tiny-7x4x20", "rr-K6",
    "tile-fp32-rk-ntw2-K64", "tile-bf16-kr-ntw1-a161-b160", "conv-fwd-n2-t3", "conv-dgrad-n5-t2", "conv-wgrad-n2-t5",
    "conv-fwd-80-512-bf16", "conv-wgrad-36-20-split-fp32")]


@pytest.mark.parametrize("c", R_CASES, ids=lambda c: c.name)
def test_r_bounds_hold_for_both_restated_orders(c):
    d = G.expected_kernel(c)
    inp = G.make_inputs(c, "R")
    for order in ("seq", "tile"):
        fails = G.judge(c, d, inp, model(c, inp, order))
        assert not fails, (order, fails)


def test_rho_of_the_restatements_is_what_the_module_says():
    """rho_rms at 64 x 64, in units of 2^-24: about 0.4 (fp32, uniform operands) and 0.9 (six-term fp32x3); a lost a1 b3 term
    shows in it only while K is small — 12.7 at K = 16, 5.7 at K = 80, 2.3 at K = 516 against 0.9: its share falls as
    1 / sqrt(K) and passes under the factor 2 of the RMS condition between K = 516 and K = 2048."""
    rs = np.random.default_rng(5)
    out = {}
    for K in (16, 80, 516):
        a, b = (rs.random((64, K)) * 2 - 1).astype(F), (rs.random((K, 64)) * 2 - 1).astype(F)
        for mode in ("fp32", "fp32x3"):
            c = G.Case(name="rho", M=64, N=64, K=K, mode=mode)
            out[(mode, K)] = G.rho_of(c, a, b, None, None, None, 128, 64)[1] / G.EPS32
        c = G.Case(name="rho", M=64, N=64, K=K, mode="fp32x3")
        out[("drop", K)] = G.rho_of(c, a, b, None, None, None, 128, 64, mut=dict(drop=(0, 2)))[1] / G.EPS32
    print({k: round(v, 2) for k, v in out.items()})
    for K in (16, 80, 516):
        assert 0.2 < out[("fp32", K)] < 0.8 and 0.7 < out[("fp32x3", K)] < 1.6
    assert out[("drop", 16)] > 2 * out[("fp32x3", 16)] and out[("drop", 80)] > 2 * out[("fp32x3", 80)]
    ratio = {K: out[("drop", K)] / out[("fp32x3", K)] for K in (16, 80, 516)}
    assert ratio[16] > ratio[80] > ratio[516] and ratio[516] < 3.0      # at the edge of the factor 2: E1 / E3 find it there


# ----------------------------------------------------------------------------------------------------- the mutants
def _caught_by(c, mut, post=None, classes=None):
    """The classes of case `c` that flag the mutated model; the unmutated model must pass every one of them first."""
    d = G.expected_kernel(c)
    hit = []
    for inp in G.iter_inputs(c, d):
        if classes and inp.cls not in classes:
            continue
        assert not G.judge(c, d, inp, model(c, inp)), (c.name, inp.cls, "the unmutated restatement fails")
        outs = model(c, inp, mut=mut)
        if post:
            outs = post(c, d, inp, outs)
        if G.judge(c, d, inp, outs) and inp.cls not in hit:
            hit.append(inp.cls)
    return hit


def _move_one_element(c, d, inp, outs):
    if inp.cls != "R":
        return outs
    a, b = G.products(c, inp.a, inp.b)[0]
    rho = G.rho_of(c, a, b, inp.bias, None, d["k_per_split"], d["bm"], d["bn"])
    z, tol, S, u = G.r_bounds(c, a, b, inp.bias, None, d["split_k"], rho[0])
    o = outs[0].astype(F64)
    o[5, 40] = z[5, 40] + 3 * tol[5, 40]
    return [o]


def _small_row_wrong(scale):
    def post(c, d, inp, outs):
        if inp.cls != "R":
            return outs
        o = outs[0].astype(F64)
        zr, sr, sc = G.r_blocks(*o.shape)
        o[sr.start + 1] += scale * np.abs(o).max()
        return [o]
    return post


MUTANTS = [
    # (number, what, case, mutation of the restatement, post-processing of its outputs, classes that must flag it)
    (1, "a1 b3 dropped", "epi-fp32x3-store", dict(drop=(0, 2)), None, {"E1"}),
    (2, "a2 b2 dropped", "epi-fp32x3-store", dict(drop=(1, 1)), None, {"E3"}),
    (3, "bf16 mode truncating instead of RNE", "epi-bf16-store", dict(trunc=True), None, {"E1"}),
    (4, "accumulator rounded to bf16 once per k-tile", "epi-fp32x3-store", dict(acc_bf16=True), None, {"E2", "E3", "R"}),
    (5, "one k skipped in the last partial k-tile", "ntw1-130x260x516", dict(skip_k=515), None, {"E1", "E2"}),
    (6, "one k-tile counted by two neighbouring splits", "epi-fp32x3-atomic-bias-split3", dict(double_tile=True), None, {"E2"}),
    (7, "one tile unwritten and another written twice", "xcd-8x3", dict(tile_map=True), None, {"E2"}),
    (8, "zero padding missing at one sequence end", "conv-fwd-n2-t3", dict(no_padding=True), None, {"E1", "E2"}),
    (9, "weight-gradient tap shift with the wrong sign", "conv-wgrad-n2-t3", dict(wgrad_sign=True), None, {"E1", "E2"}),
    (10, "bias added once per split", "epi-fp32x3-atomic-bias-split3", dict(bias_per_split=True), None, {"E2"}),
    (11, "ACCUM ignoring its base", "epi-fp32x3-accum", dict(no_base=True), None, {"E2", "R"}),
    (12, "batched product b reading product 0's B", "batched2-accum", dict(batched_b0=True), None, {"E2"}),
    (13, "one element moved by three bounds", "epi-fp32x3-store", None, _move_one_element, {"R"}),
    (14, "a 2^-12-scaled row wrong by 1e-4 of the tensor's maximum", "epi-fp32x3-store", None, _small_row_wrong(1e-4), {"R"}),
    (15, "... and by 1e-4 of its own scale (2e-8 of the maximum)", "epi-fp32x3-store", None, _small_row_wrong(1e-4 * 2.0 ** -12),
     {"R"}),
]


@pytest.mark.parametrize("num,what,case,mut,post,must", MUTANTS, ids=[f"m{m[0]}" for m in MUTANTS])
def test_mutants_are_flagged(num, what, case, mut, post, must):
    c = G.CASE_BY_NAME[case]
    hit = _caught_by(c, mut, post)
    CAUGHT[num] = (what, case, hit)
    print(f"mutant {num} ({what}) at {case}: flagged by {hit}")
    assert must <= set(hit), (what, case, hit)


def test_lost_split_term_and_the_rms_condition():
    """Mutant 1 against class R alone, on the restatement: flagged at K = 16 (per element, 3.8 bounds, and in the RMS), at
    K = 516 by the RMS alone and barely (2.1 against 1.7 eps), not at all at K = 2048 — there a lost a1 b3 rests on E1 (and a
    lost a2 b2 on E3), which flag it at every K."""
    seen = {}
    for K in (16, 516, 2048):
        c = G.Case(name=f"rms-K{K}", M=64, N=64, K=K, mode="fp32x3", classes=("R",))
        d = G.expected_kernel(c)
        inp = G.make_inputs(c, "R")
        assert not G.judge(c, d, inp, model(c, inp))
        seen[K] = G.judge(c, d, inp, model(c, inp, mut=dict(drop=(0, 2))))
    assert seen[16] and any("element" in f for f in seen[16]), "R does not see a lost a1 b3 even at K = 16"
    assert not seen[2048], "R sees a lost a1 b3 at K = 2048: the module says it does not"
    CAUGHT["1 by R alone"] = {K: bool(v) for K, v in seen.items()}
    print("mutant 1 by class R alone:", CAUGHT["1 by R alone"])
