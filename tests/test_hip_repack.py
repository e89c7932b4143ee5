"""The per-step repack launch (csrc/repack.hip: dvae_repack_all, dvae_lstm_pack_w / _bf16 / _x3) and derived.DerivedWeights
on the MI355X through the C ABI, against tests/repack_ref.py, BIT FOR BIT: every kind moves bits, rounds once to bf16 or adds
once, so there is no tolerance anywhere in this module.

Every destination is a guarded buffer of tests/kernel_harness.py (0xFF fill, 0xA5 guards), every source lies between NaNs,
every comparison covers 100 % of the elements, and the elements a kind must not write must keep the fill.  Sources are
full-significand fp32 values; the cast and transpose kinds also get +-0, subnormals, bf16 ties with their neighbours, the
largest fp32, +-inf and NaN (a NaN source is only asked to give a NaN in bf16: repack_ref.cast_bf16).  Pack sources are finite
with |w| over [2^-110, 2^120]; one x3 case with subnormal sources prints what the device does there.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import (assert_same_bits, bits, Buf, down, EINVAL, F32, guards, L, make_trainer, ok, Pad, st,  # noqa: E402
                            sync, untouched)
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib  # noqa: E402
import repack_ref as R  # noqa: E402

K = R.KINDS
F32M, BF16M, X3M = 0, 1, 2
MODES = {"fp32": F32M, "bf16": BF16M, "fp32x3": X3M}
BF = torch.bfloat16


def widen(u16):
    return (np.asarray(u16).view(np.uint16).astype(np.uint32) << 16).view(F32)


def desc(kind, src, dst, d0, d1=0, d2=0, src2=None, dst2=None):
    d = _lib.RepackDesc()
    d.kind, d.d0, d.d1, d.d2 = kind, d0, d1, d2
    d.src, d.src2, d.dst, d.dst2 = src, src2, dst, dst2
    return d


class Item:
    """One descriptor, the guarded buffers it writes and the comparison of what it left there."""

    def __init__(self, d, dsts, check, keep=()):
        self.d, self.dsts, self.check, self.keep = d, list(dsts), check, keep     # keep: the sources, alive until the launch ran


def table(items):
    return (_lib.RepackDesc * len(items))(*[i.d for i in items])


def launch(items, check=True):
    ok(L().dvae_repack_all(table(items), len(items), st()), "dvae_repack_all")
    guards(*[b for i in items for b in i.dsts])
    if check:
        for i in items:
            i.check()


def held(buf, ref, what, mask=None, nan=None):
    """`buf` holds the bits of `ref` (fp32 values, or uint16 bf16 patterns) wherever `mask` says (everywhere without one) and
    the 0xFF fill everywhere else.  nan (bf16 only): where the source was a NaN — there only a NaN is asked for."""
    if buf.esize == 4 and mask is None and nan is None:
        return assert_same_bits(buf, ref, what)
    got = buf.bits()
    g = got.view(np.uint32 if buf.esize == 4 else np.uint16).reshape(-1)
    r = (bits(ref) if buf.esize == 4 else np.asarray(ref, np.uint16)).reshape(-1)
    assert g.shape == r.shape, f"{what}: {g.size} elements instead of {r.size}"
    m = np.ones(g.shape, bool) if mask is None else np.asarray(mask, bool).reshape(-1)
    untouched(got.reshape(-1)[~m], what)
    cmp = m
    if nan is not None:
        nan = np.asarray(nan, bool).reshape(-1) & m
        assert buf.esize == 2 and np.isnan(widen(g[nan])).all(), f"{what}: a NaN source did not give a NaN"
        cmp = m & ~nan
    bad = np.nonzero((g != r) & cmp)[0]
    assert not bad.size, (f"{what}: {bad.size} of {int(cmp.sum())} elements differ in their bits, first at {bad[:1]}: "
                          f"{g[bad[:1]]} instead of {r[bad[:1]]}")


def values(rs, n, special):
    x = R.full_f32(rs, n)
    return R.with_specials(rs, x) if special else x


# ------------------------------------------------------------------ the kinds as items
def t_item(rs, R_, C, ld=0, b16=False, special=True, into=None, col0=0):
    """TRANSPOSE of a fresh source into a fresh [C][ld] destination, or into columns col0 .. col0 + R_ of `into`."""
    W = values(rs, R_ * C, special).reshape(R_, C)
    src = Pad(W)
    lde = ld or R_
    dst = into if into is not None else Buf((C, lde), BF if b16 else torch.float32)
    ref, mask = R.transpose(W, R_, C, lde, b16)
    nanm = R.transpose(np.isnan(W).astype(F32), R_, C, lde)[0] != 0
    d = desc(K["TRANSPOSE"], src.ptr, dst.at(col0), R_, C, int(b16) | (ld << 1))
    what = f"TRANSPOSE {R_}x{C} ld={ld} bf16={b16}"

    def check():
        if into is None:
            held(dst, ref, what, mask, nanm if b16 else None)
        else:                       # a shared destination: this descriptor's columns only; the caller looks at the rest
            got = dst.bits().view(np.uint16 if b16 else np.uint32)[:, col0:col0 + R_]
            want = (ref if b16 else bits(ref))[:, :R_]
            keep = ~nanm[:, :R_] if b16 else np.ones_like(nanm[:, :R_])
            assert np.array_equal(got[keep], want[keep]), what + f" at column {col0}"
            assert np.isnan(widen(got[~keep])).all() if b16 else True
    return Item(d, [dst] if into is None else [], check, (src,))


def conv_item(rs, Cout, Cin, b16=False, special=True):
    Wp = values(rs, 5 * Cout * Cin, special).reshape(5, Cout, Cin)
    src, dst = Pad(Wp), Buf((5, Cin, Cout), BF if b16 else torch.float32)
    ref = R.conv_t(Wp, Cout, Cin, b16)
    nanm = R.conv_t(np.isnan(Wp).astype(F32), Cout, Cin) != 0
    return Item(desc(K["CONV_T"], src.ptr, dst.ptr, Cout, Cin, int(b16)), [dst],
                lambda: held(dst, ref, f"CONV_T {Cout}x{Cin} bf16={b16}", None, nanm if b16 else None), (src,))


def copy_item(rs, n):
    x = R.full_f32(rs, n)
    src, dst = Pad(x), Buf((n,))
    return Item(desc(K["COPY_F32"], src.ptr, dst.ptr, n), [dst], lambda: held(dst, R.copy_f32(x), f"COPY_F32 n={n}"), (src,))


def cast_item(rs, n, rows=1, special=True):
    x = values(rs, n, special)
    src, dst = Pad(x), Buf((n,), BF)
    return Item(desc(K["CAST_BF16"], src.ptr, dst.ptr, n // rows, rows), [dst],
                lambda: held(dst, R.cast_bf16(x), f"CAST_BF16 n={n}", None, np.isnan(x)), (src,))


def add_item(rs, n, in_place=False):
    a, b = R.full_f32(rs, n), R.full_f32(rs, n)
    a[: n // 2] = -b[: n // 2] * F32(1 + 2.0 ** -20)           # cancellation: the sum's last bits come from both operands
    sb = Pad(b)
    if in_place:
        dst = Buf(data=a)
        sa = dst
    else:
        dst, sa = Buf((n,)), Pad(a)
    return Item(desc(K["ADD2"], sa.ptr, dst.ptr, n, src2=sb.ptr), [dst],
                lambda: held(dst, R.add2(a, b), f"ADD2 n={n} in_place={in_place}"), (sa, sb))


@functools.lru_cache(maxsize=None)
def pack_w(H):
    return R.pack_source(np.random.RandomState(H), H)


@functools.lru_cache(maxsize=None)
def pack_pad(H):
    return Pad(pack_w(H))


@functools.lru_cache(maxsize=None)
def pack_ref(H, mode):
    """(fwd, bwd) of pack_w(H) in `mode`, as bytes: computed once, shared, never written."""
    out = tuple(R.as_bytes(p) for p in R.PACKS[mode](pack_w(H), H))
    for o in out:
        o.setflags(write=False)
        assert o.size == R.pack_nbytes(mode, H)
    return out


def pack_buf(H, mode):
    """A pack destination as the package allocates it: 6*H*H floats (room for three planes); what lies behind a shorter pack
    must keep the fill (it counts as a guard)."""
    b = Buf((6 * H * H,))
    b.slack_from = R.pack_nbytes(mode, H)
    return b


def pack_held(buf, H, mode, which, what):
    n = R.pack_nbytes(mode, H)
    got = buf.bits().view(np.uint8)[:n]
    ref = pack_ref(H, mode)[which]
    bad = np.nonzero(got != ref)[0]
    assert not bad.size, f"{what}: {bad.size} of {n} bytes differ, first at byte {bad[:1]}"


def pack_item(H, mf, mb, fwd=True, bwd=True):
    pf, pb = (pack_buf(H, mf) if fwd else None), (pack_buf(H, mb) if bwd else None)
    d = desc(K["LSTM_PACK"], pack_pad(H).ptr, pf.ptr if fwd else None, H, mf, mb, dst2=pb.ptr if bwd else None)

    def check():
        if fwd:
            pack_held(pf, H, mf, 0, f"LSTM_PACK H={H} forward mode {mf}")
        if bwd:
            pack_held(pb, H, mb, 1, f"LSTM_PACK H={H} backward mode {mb}")
    return Item(d, [b for b in (pf, pb) if b is not None], check)


# ------------------------------------------------------------------ TRANSPOSE
@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [1, 32, 33, 70])
@pytest.mark.parametrize("R_", [1, 31, 32, 33, 65])
def test_transpose(R_, C, b16):
    rs = np.random.RandomState(1000 * R_ + C)
    for ld in (0, R_, R_ + 5):
        launch([t_item(rs, R_, C, ld, b16)])


@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
def test_transpose_two_descriptors_side_by_side_in_one_destination(b16):
    """As derived.lstm_local_pair: W_ih^T of the two directions in the halves of one [In][8H] buffer, ld = 2R."""
    R_, C = 65, 33
    for alone in (True, False):                     # a fresh destination per launch: nothing an earlier launch wrote can help
        rs = np.random.RandomState(7)
        dst = Buf((C, 2 * R_), BF if b16 else torch.float32)
        items = [t_item(rs, R_, C, 2 * R_, b16, into=dst, col0=0), t_item(rs, R_, C, 2 * R_, b16, into=dst, col0=R_)]
        run = items[1:] if alone else items
        launch(run, check=False)
        guards(dst)
        for i in run:
            i.check()
        if alone:                                   # the right half alone: the left half keeps the fill
            untouched(dst.bits()[:, :R_], "the left half while only the right one was written")


def test_transpose_beyond_the_block_clamp():
    """2048 x 2049: more than 512 * 8192 elements, 4160 tiles on 512 workgroups (the tile stride loop)."""
    assert 2048 * 2049 > R.MAX_BLOCKS * R.ELEMS_PER_BLOCK
    launch([t_item(np.random.RandomState(8), 2048, 2049)])


# ------------------------------------------------------------------ CONV_T
@pytest.mark.parametrize("b16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cout,Cin", [(1, 1), (33, 7), (32, 64), (80, 130)])
def test_conv_t(Cout, Cin, b16):
    launch([conv_item(np.random.RandomState(Cout + Cin), Cout, Cin, b16)])


# ------------------------------------------------------------------ COPY_F32 / CAST_BF16 / ADD2
SWEEPS = [4, 8188, 8192, 8196, 512 * 8192 * 4 + 4]          # the last: two sweeps of 512 workgroups and a ragged third


@pytest.mark.parametrize("n", SWEEPS)
def test_copy_f32(n):
    launch([copy_item(np.random.RandomState(n % 9973), n)])


@pytest.mark.parametrize("n", SWEEPS)
def test_cast_bf16(n):
    launch([cast_item(np.random.RandomState(n % 9973), n)])


def test_cast_bf16_counts_d0_times_d1():
    launch([cast_item(np.random.RandomState(3), 6 * 4098, rows=6)])


@pytest.mark.parametrize("n", [1, 255, 257, 8193])
def test_add2(n):
    rs = np.random.RandomState(n)
    launch([add_item(rs, n)])
    launch([add_item(rs, n, in_place=True)])


# ------------------------------------------------------------------ LSTM_PACK and the stand-alone entry points
@pytest.mark.parametrize("H", [64, 128])
def test_lstm_pack_fp32_small(H):
    launch([pack_item(H, F32M, F32M)])


@pytest.mark.parametrize("mb", list(MODES))
@pytest.mark.parametrize("mf", list(MODES))
def test_lstm_pack_512_every_pair_of_modes(mf, mb):
    launch([pack_item(512, MODES[mf], MODES[mb])])


@pytest.mark.parametrize("mode", list(MODES))
def test_lstm_pack_512_one_destination_only(mode):
    launch([pack_item(512, MODES[mode], MODES[mode], bwd=False)])
    launch([pack_item(512, MODES[mode], MODES[mode], fwd=False)])


def test_lstm_pack_1024_x3():
    launch([pack_item(1024, X3M, X3M)])


ENTRY = {F32M: "dvae_lstm_pack_w", BF16M: "dvae_lstm_pack_w_bf16", X3M: "dvae_lstm_pack_w_x3"}


@pytest.mark.parametrize("fwd,bwd", [(True, False), (False, True), (True, True)], ids=["fwd", "bwd", "both"])
@pytest.mark.parametrize("mode", list(MODES))
def test_stand_alone_pack_entry_points(mode, fwd, bwd):
    m, H = MODES[mode], 512
    pf, pb = (pack_buf(H, m) if fwd else None), (pack_buf(H, m) if bwd else None)
    ok(getattr(L(), ENTRY[m])(pack_pad(H).ptr, pf.ptr if fwd else None, pb.ptr if bwd else None, H, st()), ENTRY[m])
    guards(pf, pb)
    it = pack_item(H, m, m, fwd, bwd)
    launch([it])
    for which, (alone, tab) in enumerate(((pf, it.dsts[0] if fwd else None), (pb, it.dsts[-1] if bwd else None))):
        if alone is not None:
            pack_held(alone, H, m, which, f"{ENTRY[m]} {'bwd' if which else 'fwd'}")
            assert np.array_equal(alone.bits(), tab.bits()), "the stand-alone pack and the table's differ"


def test_stand_alone_fp32_pack_at_64():
    pf, pb = pack_buf(64, F32M), pack_buf(64, F32M)
    ok(L().dvae_lstm_pack_w(pack_pad(64).ptr, pf.ptr, pb.ptr, 64, st()))
    guards(pf, pb)
    pack_held(pf, 64, F32M, 0, "dvae_lstm_pack_w fwd H=64")
    pack_held(pb, 64, F32M, 1, "dvae_lstm_pack_w bwd H=64")


def test_x3_pack_of_subnormal_weights_is_finite(capsys):
    """Below 2^-110 "w == w1 + w2 + w3 exactly" is not promised (include/dvae_hip.h).  What the device does with fp32
    subnormals is printed, and recorded in the header comment of dvae_lstm_pack_w_x3 and in DESIGN.md section 5; only
    finiteness is asserted."""
    H = 512
    rs = np.random.RandomState(21)
    w = rs.randint(1, 1 << 23, size=4 * H * H).astype(np.uint32)
    w |= rs.randint(0, 2, size=w.size).astype(np.uint32) << 31
    w = w.view(F32).reshape(4 * H, H)
    src, pf, pb = Pad(w), pack_buf(H, X3M), pack_buf(H, X3M)
    ok(L().dvae_lstm_pack_w_x3(src.ptr, pf.ptr, pb.ptr, H, st()))
    guards(pf, pb)
    n = R.pack_nbytes(X3M, H)
    for name, buf, (plain, ref) in zip(("fwd", "bwd"), (pf, pb), zip(R._frag(w, H, 32, 8), R.pack_x3(w, H))):
        got = buf.bits().view(np.uint16)[: n // 2].reshape(ref.shape)
        planes = widen(got).astype(np.float64)
        assert np.isfinite(planes).all()
        exact = planes.sum(2) == plain.astype(np.float64)
        rne = planes[:, :, 0] == widen(R.rne16(plain)).astype(np.float64)
        with capsys.disabled():
            print(f"\nx3 pack of fp32 subnormals ({name}): equal to the IEEE split {np.array_equal(got, ref)}; planes sum to w "
                  f"exactly for {exact.mean():.4f} of the elements; plane 0 == rne(w) for {rne.mean():.4f}; plane 0 all zero "
                  f"{not planes[:, :, 0].any()}; planes 1, 2 all zero {not planes[:, :, 1:].any()}")


# ------------------------------------------------------------------ tables
def big_table(seed):
    """72 descriptors, the six kinds interleaved, from one workgroup each to the 512-workgroup clamp."""
    rs = np.random.RandomState(seed)
    shapes = {"TRANSPOSE": [(1, 1), (33, 70), (65, 33), (256, 80), (512, 512), (2048, 2049), (31, 1), (1, 300), (700, 130),
                            (96, 96), (8, 1025), (129, 64)],
              "CONV_T": [(1, 1), (33, 7), (80, 130), (512, 512), (32, 64), (7, 33), (2, 2049), (100, 3), (64, 64), (5, 5),
                         (130, 80), (17, 290)],
              "COPY_F32": [4, 8196, 100000, 512 * 8192 + 8192 + 4, 8192, 16384, 12, 40004, 8188, 24580, 300, 65536],
              "CAST_BF16": [4, 8188, 196608, 8192, 8196, 512 * 8192 + 4, 16, 81924, 1028, 24576, 40, 65540],
              "ADD2": [1, 257, 8193, 2048, 255, 8192, 16385, 3, 1000, 256, 33000, 7],
              "LSTM_PACK": [64, 128, 512, 64, 64, 128, 512, 64, 128, 64, 512, 64]}
    items = []
    for i in range(R.MAX_DESC):
        kind, k = list(shapes)[i % 6], i // 6
        s = shapes[kind][k]
        if kind == "TRANSPOSE":
            items.append(t_item(rs, s[0], s[1], (s[0] + 3) * (k % 3 == 2), k % 2 == 1))
        elif kind == "CONV_T":
            items.append(conv_item(rs, s[0], s[1], k % 2 == 0))
        elif kind == "COPY_F32":
            items.append(copy_item(rs, s))
        elif kind == "CAST_BF16":
            items.append(cast_item(rs, s))
        elif kind == "ADD2":
            items.append(add_item(rs, s))
        else:
            mf, mb = ((k % 3, (k + 1) % 3) if s == 512 else (F32M, F32M))
            items.append(pack_item(s, mf, mb, fwd=k != 4, bwd=k != 7))
    return items


def elems_of(d):
    return {K["CONV_T"]: 5 * d.d0 * d.d1, K["LSTM_PACK"]: 4 * d.d0 * d.d0, K["TRANSPOSE"]: d.d0 * d.d1, K["ADD2"]: d.d0,
            K["COPY_F32"]: d.d0, K["CAST_BF16"]: d.d0 * max(1, d.d1)}[d.kind]


def test_table_of_72_descriptors_and_a_second_launch():
    items = big_table(5)
    nb = [R.blocks_of(elems_of(i.d)) for i in items]
    assert len(items) == 72 and min(nb) == 1 and nb.count(R.MAX_BLOCKS) >= 3 and len(set(nb)) > 10
    assert {i.d.kind for i in items} == set(K.values())
    launch(items)
    first = [b.raw.clone() for i in items for b in i.dsts]
    launch(items, check=False)
    sync()
    for a, b in zip(first, [b for i in items for b in i.dsts]):
        assert torch.equal(a, b.raw), "a second launch of the same table left other bits"


def test_one_source_under_several_descriptors():
    rs = np.random.RandomState(9)
    R_, C = 70, 36
    W = R.with_specials(rs, R.full_f32(rs, R_ * C)).reshape(R_, C)
    src = Pad(W)
    t32, t16, c32, c16 = Buf((C, R_)), Buf((C, R_ + 2), BF), Buf((R_ * C,)), Buf((R_ * C,), BF)
    ds = [desc(K["TRANSPOSE"], src.ptr, t32.ptr, R_, C), desc(K["CAST_BF16"], src.ptr, c16.ptr, R_ * C, 1),
          desc(K["TRANSPOSE"], src.ptr, t16.ptr, R_, C, 1 | ((R_ + 2) << 1)), desc(K["COPY_F32"], src.ptr, c32.ptr, R_ * C)]
    ok(L().dvae_repack_all((_lib.RepackDesc * 4)(*ds), 4, st()))
    guards(t32, t16, c32, c16)
    nan = np.isnan(W)
    held(t32, R.transpose(W, R_, C)[0], "fp32 transpose")
    ref16, m16 = R.transpose(W, R_, C, R_ + 2, True)
    held(t16, ref16, "bf16 transpose", m16, R.transpose(nan.astype(F32), R_, C, R_ + 2)[0] != 0)
    held(c32, W, "copy")
    held(c16, R.cast_bf16(W), "cast", None, nan)


# ------------------------------------------------------------------ refusals: nothing is launched
def refused(bad, extra_dsts=()):
    """`bad` last in an otherwise valid table: DVAE_EINVAL, and every destination of the table keeps its fill."""
    rs = np.random.RandomState(1)
    items = [t_item(rs, 33, 5), copy_item(rs, 8), add_item(rs, 5)]
    arr = (_lib.RepackDesc * 4)(*[i.d for i in items], bad)
    assert L().dvae_repack_all(arr, 4, st()) == EINVAL
    dsts = [b for i in items for b in i.dsts] + list(extra_dsts)
    guards(*dsts)
    for b in dsts:
        assert b.poisoned().all(), "a refused table was launched"


H512 = 512
BAD = {
    # name -> (kind, d0, d1, d2, src, src2, dst, dst2); "s" a valid source, "d" / "e" valid destinations, an integer: that
    # many bytes past a valid one
    "conv_t null src": ("CONV_T", 3, 4, 0, None, None, "d", None),
    "conv_t null dst": ("CONV_T", 3, 4, 0, "s", None, None, None),
    "conv_t Cout 0": ("CONV_T", 0, 4, 0, "s", None, "d", None),
    "conv_t Cin 0": ("CONV_T", 3, 0, 0, "s", None, "d", None),
    "pack null src": ("LSTM_PACK", 64, 0, 0, None, None, "d", "e"),
    "pack no destination": ("LSTM_PACK", 64, 0, 0, "s", None, None, None),
    "pack H 32": ("LSTM_PACK", 32, 0, 0, "s", None, "d", "e"),
    "pack H 96": ("LSTM_PACK", 96, 0, 0, "s", None, "d", "e"),
    "pack bf16 fwd at H 64": ("LSTM_PACK", 64, 1, 0, "s", None, "d", "e"),
    "pack x3 bwd at H 64": ("LSTM_PACK", 64, 0, 2, "s", None, "d", "e"),
    "pack x3 fwd at H 576": ("LSTM_PACK", 576, 2, 0, "s", None, "d", "e"),
    "pack bf16 bwd at H 576": ("LSTM_PACK", 576, 0, 1, "s", None, "d", "e"),
    "pack fwd mode 3": ("LSTM_PACK", H512, 3, 0, "s", None, "d", "e"),
    "pack bwd mode 3": ("LSTM_PACK", H512, 0, 3, "s", None, "d", "e"),
    "pack mode -1": ("LSTM_PACK", H512, -1, 0, "s", None, "d", "e"),
    "pack src misaligned": ("LSTM_PACK", 64, 0, 0, 4, None, "d", "e"),
    "pack dst misaligned": ("LSTM_PACK", 64, 0, 0, "s", None, 8, "e"),
    "pack dst2 misaligned": ("LSTM_PACK", 64, 0, 0, "s", None, "d", 4),
    "transpose null src": ("TRANSPOSE", 3, 4, 0, None, None, "d", None),
    "transpose null dst": ("TRANSPOSE", 3, 4, 0, "s", None, None, None),
    "transpose R 0": ("TRANSPOSE", 0, 4, 0, "s", None, "d", None),
    "transpose C 0": ("TRANSPOSE", 3, 0, 0, "s", None, "d", None),
    "transpose d2 < 0": ("TRANSPOSE", 3, 4, -2, "s", None, "d", None),
    "transpose row stride below R": ("TRANSPOSE", 3, 4, 2 << 1, "s", None, "d", None),
    "copy null src": ("COPY_F32", 8, 0, 0, None, None, "d", None),
    "copy null dst": ("COPY_F32", 8, 0, 0, "s", None, None, None),
    "copy n 0": ("COPY_F32", 0, 0, 0, "s", None, "d", None),
    "copy n 6": ("COPY_F32", 6, 0, 0, "s", None, "d", None),
    "copy src misaligned": ("COPY_F32", 8, 0, 0, 4, None, "d", None),
    "copy dst misaligned": ("COPY_F32", 8, 0, 0, "s", None, 8, None),
    "add2 null src": ("ADD2", 5, 0, 0, None, "s", "d", None),
    "add2 null src2": ("ADD2", 5, 0, 0, "s", None, "d", None),
    "add2 null dst": ("ADD2", 5, 0, 0, "s", "s", None, None),
    "add2 n 0": ("ADD2", 0, 0, 0, "s", "s", "d", None),
    "cast null src": ("CAST_BF16", 8, 1, 0, None, None, "d", None),
    "cast null dst": ("CAST_BF16", 8, 1, 0, "s", None, None, None),
    "cast d0 0": ("CAST_BF16", 0, 1, 0, "s", None, "d", None),
    "cast d1 0": ("CAST_BF16", 8, 0, 0, "s", None, "d", None),
    "cast n 6": ("CAST_BF16", 3, 2, 0, "s", None, "d", None),
    "cast src misaligned": ("CAST_BF16", 8, 1, 0, 8, None, "d", None),
    "cast dst misaligned by 4": ("CAST_BF16", 8, 1, 0, "s", None, 4, None),
    "cast dst misaligned by 2": ("CAST_BF16", 8, 1, 0, "s", None, 2, None),
    "kind 6": (6, 8, 1, 0, "s", "s", "d", "e"),
    "kind -1": (-1, 8, 1, 0, "s", "s", "d", "e"),
}


@functools.lru_cache(maxsize=None)
def refusal_buffers():
    """One source and two destinations large enough for every entry of BAD had it been launched (H = 576, three planes)."""
    n = 6 * 576 * 576 + 64
    return Pad(np.zeros(4 * 576 * 576 + 64, F32)), Buf((n,)), Buf((n,))


@pytest.mark.parametrize("name", list(BAD))
def test_a_bad_descriptor_refuses_the_whole_table(name):
    kind, d0, d1, d2, *ptrs = BAD[name]
    s, d, e = refusal_buffers()
    base = {"s": s.ptr, "d": d.ptr, "e": e.ptr}
    src, src2 = (base["s"] + p if isinstance(p, int) else base.get(p) for p in ptrs[:2])
    dst, dst2 = (base[k] + p if isinstance(p, int) else base.get(p) for k, p in zip("de", ptrs[2:]))
    refused(desc(K.get(kind, kind), src, dst, d0, d1, d2, src2, dst2), (d, e))


def test_table_sizes_and_null_table():
    it = copy_item(np.random.RandomState(2), 8)
    arr = (_lib.RepackDesc * 73)(*[it.d] * 73)
    assert L().dvae_repack_all(None, 1, st()) == EINVAL
    assert L().dvae_repack_all(arr, 0, st()) == EINVAL
    assert L().dvae_repack_all(arr, -1, st()) == EINVAL
    assert L().dvae_repack_all(arr, 73, st()) == EINVAL
    guards(*it.dsts)
    assert it.dsts[0].poisoned().all()
    ok(L().dvae_repack_all(arr, 72, st()))            # the same copy 72 times: the largest table there is
    guards(*it.dsts)
    it.check()


@pytest.mark.parametrize("mode", list(MODES))
def test_stand_alone_entry_points_refuse(mode):
    m = MODES[mode]
    fn = getattr(L(), ENTRY[m])
    s, d, e = refusal_buffers()
    good = 64 if m == F32M else 512
    cases = [(None, d.ptr, e.ptr, good), (s.ptr, None, None, good), (s.ptr + 4, d.ptr, e.ptr, good),
             (s.ptr, d.ptr + 8, e.ptr, good), (s.ptr, d.ptr, e.ptr + 4, good), (s.ptr, None, e.ptr + 8, good),
             (s.ptr, d.ptr, e.ptr, 0), (s.ptr, d.ptr, e.ptr, -64)]
    cases += [(s.ptr, d.ptr, e.ptr, H) for H in ((32, 96) if m == F32M else (64, 576, 256))]
    for w, pf, pb, H in cases:
        assert fn(w, pf, pb, H, st()) == EINVAL, (w, pf, pb, H)
    guards(d, e)
    assert d.poisoned().all() and e.poisoned().all()


# ------------------------------------------------------------------ derived.DerivedWeights on the device
@pytest.fixture(scope="module")
def trainer():
    from dvae_amd import ops
    mode = ops.current_mode()
    w = make_trainer()
    yield w
    _REFS.clear()
    ok(L().dvae_set_compute_mode(mode))


def tbits(t):
    """The bits of a device tensor (any view), as uint32 / uint16."""
    t = t.detach().contiguous()
    return down(t.view({4: torch.int32, 2: torch.int16}[t.element_size()])).view({4: np.uint32, 2: np.uint16}[t.element_size()])


def same(t, ref, what, dtype):
    """Device tensor `t` has dtype `dtype` and the bits of `ref` (fp32 values or uint16 patterns)."""
    assert t.dtype == dtype, f"{what}: {t.dtype}"
    g = tbits(t)
    r = bits(ref) if dtype == torch.float32 else np.asarray(ref, np.uint16)
    assert g.size == r.size, f"{what}: {g.size} elements instead of {r.size}"
    bad = np.nonzero(g.reshape(-1) != r.reshape(-1))[0]
    assert not bad.size, f"{what}: {bad.size} of {r.size} elements differ in their bits, first at {bad[:1]}"


_REFS = {}


def ref_of(fn, arr, *args):
    """fn(arr, *args), computed once per distinct content of `arr` (the key holds the bytes themselves: most states of the
    model below share their weights, and the three-plane packs of a 1024-unit layer are the module's longest step)."""
    key = (fn.__name__, args, arr.shape, arr.tobytes())
    if key not in _REFS:
        _REFS[key] = fn(arr, *args)
    return _REFS[key]


def derived_held(model, mode):
    """Every buffer of model._derived equals repack_ref of the parameter it is named after, as it is NOW."""
    from dvae_amd.derived import lstm_pack_modes
    d = model._derived
    b16 = mode == BF16M
    wdt = BF if b16 else torch.float32
    assert 0 < len(d._descs) <= R.MAX_DESC
    assert set(d.wpt) == set(d._convs) and set(d.lstm) == set(d._lstms) and set(d.w16) == (set(d._casts) if b16 else set())
    for name, wp in d._convs.items():
        _, cout, cin = wp.shape
        same(d.wpt[name], ref_of(R.conv_t, down(wp.detach()), cout, cin, b16), f"wpt[{name}]", wdt)
    for name, w16 in d.w16.items():
        same(w16, ref_of(R.cast_bf16, down(d._casts[name].detach())), f"w16[{name}]", BF)
        assert w16.shape == d._casts[name].shape
    seen = set()
    for name, ps in d._lstms.items():
        w_ih, w_hh, b_ih, b_hh = (down(p.detach()) for p in ps)
        H, In = w_hh.shape[1], w_ih.shape[1]
        der = d.lstm[name]
        same(der.bias, R.add2(b_ih, b_hh), f"{name}.bias", torch.float32)
        same(der.w_hh_t, ref_of(R.transpose, w_hh, 4 * H, H)[0], f"{name}.w_hh_t", torch.float32)
        wit = ref_of(R.transpose, w_ih, 4 * H, In, 0, b16)[0]
        wcopy = ref_of(R.cast_bf16, w_ih) if b16 else R.copy_f32(w_ih)
        if der.cat is not None:
            dn = int(name.rsplit(".", 1)[1])
            rows = slice(dn * 4 * H, (dn + 1) * 4 * H)
            assert H == 64 and der.w_ih_t is None and der.pack_f is None and der.pack_b is None
            assert der.cat.w_ih.shape == (8 * H, In) and der.cat.w_ih_t.shape == (In, 8 * H) and der.cat.bias.shape == (8 * H,)
            assert der.bias.data_ptr() == der.cat.bias[rows].data_ptr()
            same(der.cat.w_ih_t[:, rows], wit, f"{name}: its half of cat.w_ih_t", wdt)
            same(der.cat.w_ih[rows], wcopy, f"{name}: its half of cat.w_ih", wdt)
            assert (der.w_ih16 is None) if not b16 else der.w_ih16.data_ptr() == der.cat.w_ih[rows].data_ptr()
            seen.add((id(der.cat), dn))
            continue
        same(der.w_ih_t, wit, f"{name}.w_ih_t", wdt)
        if b16:
            same(der.w_ih16, wcopy, f"{name}.w_ih16", BF)
        else:
            assert der.w_ih16 is None
        if H % 512:
            assert der.pack_f is None and der.pack_b is None
            continue
        for which, (buf, m) in enumerate(zip((der.pack_f, der.pack_b), lstm_pack_modes(mode, H))):
            n = R.pack_nbytes(m, H)
            assert buf.numel() == 6 * H * H
            ref = R.as_bytes(ref_of(R.PACKS[m], w_hh, H)[which])
            got = down(buf.view(torch.uint8)[:n])
            assert np.array_equal(got, ref), f"{name}.pack_{'b' if which else 'f'} in mode {m}"
    cats = {c for c, _ in seen}
    assert all((c, 0) in seen and (c, 1) in seen for c in cats) and len(cats) >= 1      # both halves of every pair
    Hs = {ps[1].shape[1] for ps in d._lstms.values()}
    assert {64, 512, 1024} <= Hs


def one_forward_is_one_refresh(w):
    from oracle.fill import synthetic_pair
    x1, _ = synthetic_pair(w.batch_size, 64, 5)
    r0 = w.model._derived.refreshes
    w.model.eval()
    try:
        with torch.no_grad():
            w.model.encode_heads(x1.cuda())
    finally:
        w.model.train()
    assert w.model._derived.refreshes == r0 + 1


def refreshed(w, mode_name, held=True):
    from dvae_amd import ops
    ops.set_compute_dtype(mode_name)
    w.model._refresh_derived()
    if held:
        derived_held(w.model, MODES[mode_name])
        one_forward_is_one_refresh(w)


@pytest.mark.parametrize("mode", list(MODES))
def test_derived_weights_in_each_compute_mode(trainer, mode):
    refreshed(trainer, mode)


def test_derived_weights_follow_a_change_of_mode(trainer):
    sigs = []
    for mode in ("fp32x3", "bf16", "fp32", "fp32x3"):
        refreshed(trainer, mode)
        sigs.append(trainer.model._derived._sig)
    assert sigs[0] == sigs[3] and len(set(sigs)) == 3


def test_derived_weights_after_a_training_step_reuse_the_table(trainer):
    from oracle.fill import synthetic_pair
    w = trainer
    refreshed(w, "fp32x3", held=False)
    d = w.model._derived
    sig, descs, r0 = d._sig, d._descs, d.refreshes
    before = down(w.optimizer.flat_p)
    x1, x2 = synthetic_pair(w.batch_size, 64, 11)
    w.step(x1.cuda(), x2.cuda(), None, train=True)
    assert d.refreshes == r0 + 1                                  # one per forward
    assert not np.array_equal(bits(before), bits(down(w.optimizer.flat_p))), "the step did not move the weights"
    w.model._refresh_derived()
    assert d._sig == sig and d._descs is descs, "the weights moved in place: the table must be reused"
    _REFS.clear()
    derived_held(w.model, X3M)
    one_forward_is_one_refresh(w)


def test_derived_weights_under_the_weight_average_and_back(trainer):
    from oracle.fill import synthetic_pair
    w = trainer
    refreshed(w, "fp32x3", held=False)
    _REFS.clear()
    opt, d = w.optimizer, w.model._derived
    opt.set_ema(0.5, reset=opt.ema is not None)
    x1, x2 = synthetic_pair(w.batch_size, 64, 12)
    w.step(x1.cuda(), x2.cuda(), None, train=True)
    w.model._refresh_derived()
    sig, live = d._sig, {k: tbits(v) for k, v in d.wpt.items()}
    opt.swap_ema()
    try:
        w.model._refresh_derived()
        derived_held(w.model, X3M)                                # ... of the average, which the parameters now read
        assert d._sig == sig
        assert any(not np.array_equal(live[k], tbits(v)) for k, v in d.wpt.items()), "the average equals the weights"
        one_forward_is_one_refresh(w)
    finally:
        opt.swap_ema()
    w.model._refresh_derived()
    derived_held(w.model, X3M)
    assert d._sig == sig and all(np.array_equal(live[k], tbits(v)) for k, v in d.wpt.items())
    opt.set_ema(None)


def test_derived_weights_are_rebuilt_when_the_optimiser_rehomes_the_parameters(trainer):
    from dvae_amd.optim import FlatAdam
    w = trainer
    refreshed(w, "bf16", held=False)
    _REFS.clear()
    d = w.model._derived
    sig, descs = d._sig, d._descs
    opt = FlatAdam(w.model.backward_param_order(), lr=w.lr, layout=w.model)      # new flat buffers: every data_ptr changes
    opt.set_store_first(w.model.store_first_params(w.batch_size))
    w.optimizer = opt
    opt.flat_p.mul_(1.5)                                          # ... and other weights, so that an old buffer shows
    w.model._refresh_derived()
    assert d._sig != sig and d._descs is not descs
    derived_held(w.model, BF16M)                                  # ... of the new weights: no buffer holds the old ones
    one_forward_is_one_refresh(w)
    refreshed(w, "fp32x3", held=False)
    _REFS.clear()
