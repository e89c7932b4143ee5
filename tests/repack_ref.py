"""What the per-step repack launch (csrc/repack.hip: dvae_repack_all and the three stand-alone dvae_lstm_pack_w* entry points)
must produce, restated from include/dvae_hip.h and the layout sentences at the head of csrc/repack.hip.  numpy only.  Not a
test module: tests/test_repack_ref.py checks it on the CPU, tests/test_hip_repack.py holds the kernels to it bit for bit.

Everything here moves bits, rounds once (fp32 -> bf16, to nearest even) or adds once, so there is no bound: fp32 results are
fp32 arrays whose BITS count, bf16 results are uint16 bit patterns (`bits16`).

The fragment packs are written as reshapes and axis permutations of the documented sentences, e.g. the bf16 forward pack
    fwd: [(g*n_j+jb)][kc][lane][8] <- W[g*H + jb*16 + r][32kc + 8q + j],   lane = q*16 + r
names the row of W by (g, jb, r) and its column by (kc, q, j): W.reshape(4, n_j, 16, H/32, 4, 8) has exactly those six axes,
and the destination orders them (g, jb, kc, q, r, j).  No index arithmetic of the kernel appears.
"""
import numpy as np

from ref_common import bf16, split3

F = np.float32
KINDS = {"CONV_T": 0, "LSTM_PACK": 1, "TRANSPOSE": 2, "ADD2": 3, "CAST_BF16": 4, "COPY_F32": 5}     # DVAE_REPACK_*
MAX_DESC = 72                    # entries of one table
ELEMS_PER_BLOCK, MAX_BLOCKS = 8192, 512     # a descriptor gets ceil(elements / 8192) workgroups, at most 512


def bits16(x):
    """The bf16 bit patterns (uint16) of fp32 values that ARE bf16 values (low half zero)."""
    u = np.ascontiguousarray(x, F).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def rne16(x):
    """fp32 -> bf16 to nearest even, as bit patterns."""
    return bits16(bf16(x))


# ------------------------------------------------------------------ element kinds
def conv_t(Wp, Cout, Cin, b16=False):
    """CONV_T: Wp[5][Cout][Cin] -> Wpt[5][Cin][Cout] (fp32, or bf16 bit patterns)."""
    out = np.ascontiguousarray(np.asarray(Wp, F).reshape(5, Cout, Cin).transpose(0, 2, 1))
    return rne16(out) if b16 else out


def transpose(W, R, C, ld=0, b16=False):
    """TRANSPOSE: W[R][C] -> W^T in a destination of C rows of stride ld (0: R).  Returns (values [C][ld], mask [C][ld]): the
    mask marks the C x R elements the kind may write; the values elsewhere are 0 and mean nothing."""
    ld = ld or R
    assert ld >= R
    vals = np.zeros((C, ld), F)
    mask = np.zeros((C, ld), bool)
    vals[:, :R] = np.asarray(W, F).reshape(R, C).T
    mask[:, :R] = True
    return (rne16(vals) if b16 else vals), mask


def add2(a, b):
    """ADD2: one fp32 addition."""
    return (np.asarray(a, F) + np.asarray(b, F)).astype(F)


def copy_f32(x):
    return np.array(x, F, copy=True)


def cast_bf16(x):
    """CAST_BF16: same layout, rounded to nearest even, as bit patterns.  (A NaN source: see ref_common.bf16 — a payload in
    the low half turns into inf here, the hardware returns a quiet NaN; the tests only ask for a NaN there.)"""
    return rne16(x)


# ------------------------------------------------------------------ fragment packs of W_hh [4H][H]
def _frag(W, H, kdepth, per_lane):
    """(fwd, bwd) in fp32, both [groups][kc][lane = q*16 + r][per_lane], for chunks of kdepth = 4 * per_lane columns.
    fwd: [(g*n_j+jb)][kc][lane][e] <- W[g*H + jb*16 + r][kdepth*kc + per_lane*q + e]
    bwd: [(jb*4+w)][kc][lane][e]   <- W[w*H + kdepth*kc + per_lane*q + e][jb*16 + r]"""
    W = np.asarray(W, F).reshape(4 * H, H)
    n_j, nkc = H // 16, H // kdepth
    assert H % 16 == 0 and H % kdepth == 0 and kdepth == 4 * per_lane
    # rows (g, jb, r), columns (kc, q, e) -> (g, jb, kc, q, r, e)
    fwd = W.reshape(4, n_j, 16, nkc, 4, per_lane).transpose(0, 1, 3, 4, 2, 5)
    # rows (w, kc, q, e), columns (jb, r) -> (jb, w, kc, q, r, e)
    bwd = W.reshape(4, nkc, 4, per_lane, n_j, 16).transpose(4, 0, 1, 2, 5, 3)
    shape = (4 * n_j, nkc, 64, per_lane)
    return np.ascontiguousarray(fwd).reshape(shape), np.ascontiguousarray(bwd).reshape(shape)


def pack_f32(W, H):
    """dvae_lstm_pack_w: 16-deep chunks, four consecutive k per lane; fp32 [4 n_j][H/16][64][4] each."""
    return _frag(W, H, 16, 4)


def pack_bf16(W, H):
    """dvae_lstm_pack_w_bf16: 32-deep chunks, eight consecutive k per lane, rounded; uint16 [4 n_j][H/32][64][8] each."""
    f, b = _frag(W, H, 32, 8)
    return rne16(f), rne16(b)


def pack_x3(W, H):
    """dvae_lstm_pack_w_x3: as the bf16 pack with three planes per (group, chunk): [..][kc][plane][lane][8], plane 0 = rne(w),
    plane 1 = rne(w - p0), plane 2 = w - p0 - p1; uint16 [4 n_j][H/32][3][64][8] each."""
    return tuple(np.stack([bits16(p) for p in split3(x)], axis=2) for x in _frag(W, H, 32, 8))


PACKS = {0: pack_f32, 1: pack_bf16, 2: pack_x3}              # by DVAE_MODE_*
def pack_nbytes(mode, H):
    """Bytes of one pack: 4H*H elements of 4, 2 or 3 * 2 bytes."""
    return {0: 16, 1: 8, 2: 24}[mode] * H * H


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def blocks_of(elems):
    """Workgroups dvae_repack_all gives a descriptor of `elems` elements."""
    return int(min(MAX_BLOCKS, max(1, -(-elems // ELEMS_PER_BLOCK))))


# ------------------------------------------------------------------ inputs
SPECIALS = np.array([0x00000000, 0x80000000,                               # +-0
                     0x00000001, 0x807FFFFF, 0x00400000, 0x00008000,         # fp32 subnormals
                     0x3F808000, 0x3F807FFF, 0x3F808001,                     # a tie that rounds DOWN to even, and neighbours
                     0x3F818000, 0x3F817FFF, 0x3F818001,                     # a tie that rounds UP to even, and neighbours
                     0xBF808000, 0xBF818000,
                     0x7F7FFFFF, 0xFF7FFFFF,                                 # rounds to bf16 +-inf
                     0x7F800000, 0xFF800000,                                 # +-inf
                     0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0x7FA00000], np.uint32)   # NaN (one with its payload in the low half)


def full_f32(rs, n, lo=-20, hi=20):
    """n fp32 values with random 23-bit fractions, random signs and exponents 2^lo .. 2^hi (finite, normal)."""
    frac = rs.randint(0, 1 << 23, size=n, dtype=np.int64).astype(np.uint32)
    exp = (rs.randint(lo, hi + 1, size=n) + 127).astype(np.uint32)
    sign = rs.randint(0, 2, size=n).astype(np.uint32)
    return ((sign << 31) | (exp << 23) | frac).view(F)


def with_specials(rs, x):
    """x with SPECIALS written at random places (every one of them when x has room)."""
    x = np.array(x, F, copy=True).reshape(-1)
    k = min(len(SPECIALS), x.size)
    if x.size <= 4096:
        where = rs.permutation(x.size)[:k]
    else:                            # no permutation of millions of places: the first k distinct draws
        draws = rs.randint(0, x.size, size=8 * k)
        where = draws[np.sort(np.unique(draws, return_index=True)[1])][:k]
    assert len(set(where.tolist())) == k
    x.view(np.uint32)[where] = SPECIALS[:k]
    return x


def pack_source(rs, H):
    """W_hh [4H][H] for a pack: finite, |w| over the whole of [2^-110, 2^120]."""
    w = full_f32(rs, 4 * H * H, -110, 119).reshape(4 * H, H)
    w.reshape(-1)[:4] = F([2.0 ** -110, -2.0 ** -110, 2.0 ** 120, -2.0 ** 120])
    return w
