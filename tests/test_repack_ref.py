"""tests/repack_ref.py (what tests/test_hip_repack.py holds csrc/repack.hip to) against independent forms, on the CPU: numpy /
torch transposes and casts, scalar loops written straight from the header's layout sentences, and a read-back of the bf16
fragment packs through the operand lane map of v_mfma_f32_16x16x32_bf16 that must reproduce W @ h and W^T @ dg exactly."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repack_ref as R  # noqa: E402
from ref_common import bf16, split3  # noqa: E402

F, F64 = np.float32, np.float64


def widen(u16):
    """bf16 bit patterns -> fp32 values."""
    return (np.asarray(u16, np.uint16).astype(np.uint32) << 16).view(F)


def torch_bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, F)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(R.as_bytes(a), R.as_bytes(b))


# ------------------------------------------------------------------ element kinds
@pytest.mark.parametrize("R_,C", [(1, 1), (31, 33), (65, 70), (256, 80)])
def test_transpose_is_numpy_T_and_its_mask_covers_C_by_R(R_, C):
    rs = np.random.RandomState(R_ * 100 + C)
    W = R.full_f32(rs, R_ * C).reshape(R_, C)
    v, m = R.transpose(W, R_, C)
    assert same(v, np.ascontiguousarray(W.T)) and m.all() and m.shape == (C, R_)
    v16, m16 = R.transpose(W, R_, C, b16=True)
    assert same(v16, torch_bf16_bits(W.T)) and m16.all()
    for ld in (R_ + 5, 2 * R_):
        v, m = R.transpose(W, R_, C, ld)
        assert v.shape == m.shape == (C, ld) and int(m.sum()) == C * R_
        assert m[:, :R_].all() and not m[:, R_:].any()
        assert same(v[:, :R_], np.ascontiguousarray(W.T))
        v16, m16 = R.transpose(W, R_, C, ld, b16=True)
        assert np.array_equal(m16, m) and same(v16[:, :R_], torch_bf16_bits(W.T))
    with pytest.raises(AssertionError):
        R.transpose(np.zeros((2, 3)), 2, 3, 1)                # a row stride below R


@pytest.mark.parametrize("Cout,Cin", [(1, 1), (33, 7), (80, 130)])
def test_conv_t_is_a_permute_of_the_last_two_axes(Cout, Cin):
    rs = np.random.RandomState(Cout)
    Wp = R.full_f32(rs, 5 * Cout * Cin).reshape(5, Cout, Cin)
    ref = torch.from_numpy(Wp).permute(0, 2, 1).contiguous()
    assert same(R.conv_t(Wp, Cout, Cin), ref.numpy())
    assert same(R.conv_t(Wp.reshape(-1), Cout, Cin, b16=True), ref.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    for tap in range(5):
        assert same(R.conv_t(Wp, Cout, Cin)[tap], np.ascontiguousarray(Wp[tap].T))


def test_cast_bf16_is_torchs_cast_on_the_special_values():
    x = R.SPECIALS.view(F)
    nan = np.isnan(x)
    assert nan.sum() == 4 and len(x) == 22
    got, ref = R.cast_bf16(x), torch_bf16_bits(x)
    assert np.array_equal(got[~nan], ref[~nan])
    assert np.isnan(widen(ref[nan])).all()            # torch keeps a NaN a NaN; the integer form need not (ref_common.bf16)
    by = dict(zip(R.SPECIALS.tolist(), got.tolist()))
    assert by[0x3F808000] == 0x3F80 and by[0x3F818000] == 0x3F82            # ties: down to even, up to even
    assert by[0x3F807FFF] == 0x3F80 and by[0x3F808001] == 0x3F81 and by[0x3F817FFF] == 0x3F81 and by[0x3F818001] == 0x3F82
    assert by[0x7F7FFFFF] == 0x7F80 and by[0xFF7FFFFF] == 0xFF80            # the largest fp32 rounds to inf
    assert by[0x00000000] == 0x0000 and by[0x80000000] == 0x8000
    assert by[0x00000001] == 0x0000 and by[0x807FFFFF] == 0x8080 and by[0x00400000] == 0x0040 and by[0x00008000] == 0x0000
    rs = np.random.RandomState(3)
    y = R.with_specials(rs, R.full_f32(rs, 100000, -126, 127))
    keep = ~np.isnan(y)
    assert np.array_equal(R.cast_bf16(y)[keep], torch_bf16_bits(y)[keep])
    assert same(R.copy_f32(y), y) and R.copy_f32(y) is not y


def test_add2_is_one_fp32_addition():
    rs = np.random.RandomState(5)
    a, b = R.full_f32(rs, 5000), R.full_f32(rs, 5000)
    assert same(R.add2(a, b), (a.astype(F64) + b.astype(F64)).astype(F))      # the float64 sum of two fp32 values is exact ...
    assert R.add2(a, b).dtype == F                                           # ... up to one rounding when it is narrowed


def test_block_counts():
    assert [R.blocks_of(n) for n in (1, 8192, 8193, 512 * 8192, 512 * 8192 + 1, 1 << 30)] == [1, 1, 2, 512, 512, 512]
    assert R.MAX_DESC == 72 and sorted(R.KINDS.values()) == list(range(6))


# ------------------------------------------------------------------ fragment packs
def loop_pack(W, H, kdepth, per):
    """Straight from the sentences, one (group, chunk, lane) at a time:
    fwd: [(g*n_j+jb)][kc][lane][e] <- W[g*H + jb*16 + r][kdepth*kc + per*q + e];
    bwd: [(jb*4+w)][kc][lane][e] <- W[w*H + kdepth*kc + per*q + e][jb*16 + r]   (lane = q*16 + r)"""
    n_j, nkc = H // 16, H // kdepth
    fwd, bwd = np.empty((4 * n_j, nkc, 64, per), W.dtype), np.empty((4 * n_j, nkc, 64, per), W.dtype)
    for grp in range(4 * n_j):
        g, jb = grp // n_j, grp % n_j
        jb2, w = grp // 4, grp % 4
        for kc in range(nkc):
            for lane in range(64):
                q, r = lane // 16, lane % 16
                k0 = kdepth * kc + per * q
                fwd[grp, kc, lane] = W[g * H + jb * 16 + r, k0:k0 + per]
                bwd[grp, kc, lane] = W[w * H + k0:w * H + k0 + per, jb2 * 16 + r]
    return fwd, bwd


_W = {}


def source(H):
    if H not in _W:
        _W[H] = R.pack_source(np.random.RandomState(H), H)
    return _W[H]


@pytest.mark.parametrize("H", [64, 512])
def test_pack_f32_equals_the_scalar_loops(H):
    W = source(H)
    (f, b), (lf, lb) = R.pack_f32(W, H), loop_pack(W, H, 16, 4)
    assert f.shape == (H // 4, H // 16, 64, 4) and f.nbytes == R.pack_nbytes(0, H)
    assert same(f, lf) and same(b, lb)
    assert same(np.sort(f.reshape(-1)), np.sort(W.reshape(-1)))       # a permutation of W


def test_pack_bf16_and_x3_equal_the_scalar_loops_at_512():
    H = 512
    W = source(H)
    lf, lb = loop_pack(W, H, 32, 8)
    f, b = R.pack_bf16(W, H)
    assert f.dtype == np.uint16 and f.shape == (128, 16, 64, 8) and f.nbytes == R.pack_nbytes(1, H)
    assert same(f, torch_bf16_bits(lf)) and same(b, torch_bf16_bits(lb))
    for got, loop in zip(R.pack_x3(W, H), (lf, lb)):
        assert got.dtype == np.uint16 and got.shape == (128, 16, 3, 64, 8) and got.nbytes == R.pack_nbytes(2, H)
        p0 = torch_bf16_bits(loop)
        r1 = loop - widen(p0)
        p1 = torch_bf16_bits(r1)
        p2 = torch_bf16_bits(r1 - widen(p1))
        for p, ref in enumerate((p0, p1, p2)):
            assert same(np.ascontiguousarray(got[:, :, p]), ref), f"plane {p}"


def mfma_a_operand(frag):
    """[.., 64 lanes, 8] -> [.., 16 rows, 32 k]: lane l holds k = 8 (l >> 4) + j, j = 0..7, of row l & 15 (the A / B operand
    layout of v_mfma_f32_16x16x32_bf16)."""
    a = np.full(frag.shape[:-2] + (16, 32), np.nan, F64)
    for l in range(64):
        for j in range(8):
            a[..., l & 15, 8 * (l >> 4) + j] = frag[..., l, j]
    assert not np.isnan(a).any()
    return a


@pytest.mark.parametrize("mode", ["bf16", "x3"])
def test_packs_read_back_through_the_mfma_lane_map_give_the_products(mode):
    H, n_j, nkc = 512, 32, 16
    rs = np.random.RandomState(11)
    hi = 100 if mode == "bf16" else 1 << 22                  # integers: exact in bf16 / in three planes
    W = rs.randint(-hi, hi + 1, size=(4 * H, H)).astype(F)
    h, dg = rs.randint(-8, 9, size=H).astype(F64), rs.randint(-8, 9, size=4 * H).astype(F64)
    if mode == "bf16":
        f, b = (widen(p).astype(F64) for p in R.pack_bf16(W, H))
    else:
        f, b = (widen(p).astype(F64).sum(2) for p in R.pack_x3(W, H))       # the three products of one chunk accumulate
    af = mfma_a_operand(f).reshape(4, n_j, nkc, 16, 32)      # group g*n_j + jb: rows jb*16 .. +16 of gate g
    out = np.einsum("gjkrc,kc->gjr", af, h.reshape(nkc, 32)).reshape(4 * H)
    assert np.array_equal(out, W.astype(F64) @ h)
    ab = mfma_a_operand(b).reshape(n_j, 4, nkc, 16, 32)      # group jb*4 + w: rows jb*16 .. +16 of W_w^T
    dh = np.einsum("jwkrc,wkc->jr", ab, dg.reshape(4, nkc, 32)).reshape(H)
    assert np.array_equal(dh, W.astype(F64).T @ dg)


def test_x3_planes_are_bf16_values_that_sum_to_w_exactly():
    H = 512
    W = source(H)
    aw = np.abs(W)
    assert aw.min() == F(2.0 ** -110) and aw.max() == F(2.0 ** 120)
    for got, plain in zip(R.pack_x3(W, H), R._frag(W, H, 32, 8)):
        planes = widen(got)                                  # widen() takes any uint16: each plane IS a bf16 value
        assert np.array_equal(got[:, :, 0], R.rne16(plain))
        assert np.array_equal(planes.astype(F64).sum(2), plain.astype(F64))
    # below 2^-110 the third residual has bits under bf16's smallest subnormal (2^-133): no longer exact in general
    x = F([2.0 ** -111 * (1 + 2.0 ** -23)])
    assert sum(p.astype(F64) for p in split3(x))[0] != F64(x[0])
    assert same(bf16(x), split3(x)[0])
