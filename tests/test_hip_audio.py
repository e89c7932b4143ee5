"""The audio kernels of csrc/frontend.hip on the MI355X through the C ABI, one entry point per launch, against the float64
reference of tests/audio_ref.py, element by element.

What audio_ref derives as bit-exact is compared bit for bit (the frames, every class-E case, the zero phase, the |a| = 0
branch, the clips, the floor, zero fills, copies, the volume partials), everything else within the rounding bounds derived
there from eps32 = 2^-24, the operation counts and the measured device-function constants, at 100 % of the elements.  Every
buffer a launch may write is a guarded one of tests/kernel_harness.py (an unwritten fp32 keeps the bits 0xFFFFFFFF); every
region an entry point must not read holds NaN (`Pad`: NaN in front of and behind every input, in the gaps of every leading
dimension).  The worst error / bound per kernel and quantity is printed at the module's end.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import assert_same_bits, Buf, EINVAL, F32, F64, guards, ibuf, L, ok, Pad, st, untouched, Worst
import dvae_amd  # noqa: E402,F401
import audio_ref as A  # noqa: E402
from test_audio_ref import (PARAMS, dtw_r_case, gl_phase_case, log_power_case, ola_case, voicing_r_case)  # noqa: E402

WORST = Worst("test_hip_audio.py", sort=True, ratio_fn=A.worst_ratio)
note = WORST.note
I64 = torch.int64


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


# ------------------------------------------------------------------ stft_frames
@pytest.mark.parametrize("integer", [True, False], ids=["E", "R"])
@pytest.mark.parametrize("fsize,hop,left,n", A.CASES["frames"])
def test_stft_frames(fsize, hop, left, n, integer):
    rs = np.random.RandomState(n + fsize)
    M = A.frames_count(n, fsize, hop, left)
    wav = rs.randint(-8, 9, n).astype(F32) if integer else A.rfull(rs, (n,))
    win = (2.0 ** rs.randint(-2, 3, fsize)).astype(F32) if integer else A.rfull(rs, (fsize,))
    bw, bwin, out = Pad(wav), Pad(win), Buf((M, fsize))
    ok(L().dvae_stft_frames(bw.ptr, n, bwin.ptr, out.ptr, M, fsize, hop, left, st()))
    guards(out)
    assert_same_bits(out, A.frames_ref(wav, win, A.seg_table([M], [n]), M, fsize, hop, left), f"stft_frames {fsize}/{hop} left={left} n={n}")


@pytest.mark.parametrize("fsize,hop,left,ns", A.CASES["frames_seg"])
def test_stft_frames_seg(fsize, hop, left, ns):
    rs = np.random.RandomState(fsize)
    Ms = [A.frames_count(n, fsize, hop, left) for n in ns]
    seg, rows = A.seg_table(Ms, ns), sum(Ms)
    wav, win = A.rfull(rs, (sum(ns),)), A.rfull(rs, (fsize,))
    bw, bwin, bs, out = Pad(wav), Pad(win), ibuf(seg), Buf((rows, fsize))
    ok(L().dvae_stft_frames_seg(bw.ptr, bs.ptr, len(ns), rows, bwin.ptr, out.ptr, fsize, hop, left, st()))
    guards(out)
    assert_same_bits(out, A.frames_ref(wav, win, seg, rows, fsize, hop, left), f"stft_frames_seg {fsize}/{hop}")


# ------------------------------------------------------------------ magnitude, gl_init, gl_phase
@pytest.mark.parametrize("rows,nbp", A.CASES["rows_nbp"])
def test_stft_magnitude(rows, nbp):
    rs = np.random.RandomState(rows)
    x = A.rfull(rs, (rows, 2 * nbp))
    bx, out = Pad(x), Buf((rows, nbp))
    ok(L().dvae_stft_magnitude(bx.ptr, out.ptr, rows, nbp, st()))
    guards(out)
    ref, tol = A.magnitude_bounds(x, nbp)
    note("stft_magnitude", out.np(), ref, tol, f"rows={rows} nbp={nbp}")
    e = np.zeros((rows, 2 * nbp), F32)                                   # class E: 3-4-5 triangles scaled by powers of two
    sc = (2.0 ** rs.randint(-3, 4, (rows, nbp))).astype(F32)
    e[:, :nbp], e[:, nbp:] = 3 * sc, -4 * sc
    be, oe = Pad(e), Buf((rows, nbp))
    ok(L().dvae_stft_magnitude(be.ptr, oe.ptr, rows, nbp, st()))
    guards(oe)
    assert_same_bits(oe, 5 * sc, "stft_magnitude class E")


@pytest.mark.parametrize("rows,nbp", A.CASES["rows_nbp"])
def test_gl_init(rows, nbp):
    rs = np.random.RandomState(rows + 1)
    mag, ph = np.abs(A.rfull(rs, (rows, nbp))), rs.uniform(-64, 64, (rows, nbp)).astype(F32)
    ph.reshape(-1)[0] = 0.0
    bm, bp = Pad(mag), Pad(ph)
    out = Buf((rows, 2 * nbp))
    ok(L().dvae_gl_init(bm.ptr, None, out.ptr, rows, nbp, st()))
    guards(out)
    assert_same_bits(out, np.concatenate([mag, np.zeros_like(mag)], 1), "gl_init without a phase")
    out = Buf((rows, 2 * nbp))
    ok(L().dvae_gl_init(bm.ptr, bp.ptr, out.ptr, rows, nbp, st()))
    guards(out)
    ref, tol = A.gl_init_bounds(mag, ph)
    note("gl_init", out.np(), ref, tol, f"rows={rows} nbp={nbp}")


@pytest.mark.parametrize("rows,nbp", A.CASES["rows_nbp"])
def test_gl_phase(rows, nbp):
    rs = np.random.RandomState(rows + 2)
    reb, prev, mag = gl_phase_case(rs, rows, nbp)
    br, bp, bm = Pad(reb), Pad(prev), Pad(mag)
    for pv, bpv, mom in ((prev, bp, 0.99), (None, None, 0.99), (prev, bp, 0.0)):
        out = Buf((rows, 2 * nbp))
        ok(L().dvae_gl_phase(br.ptr, None if bpv is None else bpv.ptr, bm.ptr, out.ptr, rows, nbp, mom, st()))
        guards(out)
        ref, tol, zero = A.gl_phase_bounds(reb, pv, mag, nbp, mom)
        got = out.np()
        note("gl_phase", got, ref, tol, f"rows={rows} nbp={nbp} prev={pv is not None} momentum={mom}")
        assert_same_bits(got[zero], ref[zero].astype(F32), "gl_phase where |a| = 0: (mag, +0)")
        if pv is not None and mom > 0:
            assert zero.any()


# ------------------------------------------------------------------ the dB transposes
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("M,C", A.CASES["transpose"])
def test_mel_db_normalize(M, C, pname):
    rs = np.random.RandomState(M * 100 + C)
    ml, rdb, mdb = PARAMS[pname]
    x = A.db_edge_values(rs, M, C, ml, rdb, mdb)
    x.reshape(-1)[rs.randint(0, x.size)] = F32(ml) / 2                   # below the floor
    ref, tol, _ = A.db_normalize_bounds(x, ml, rdb, mdb)
    bx = Pad(x)
    for ld, col0 in ((M, 0), (M + 7, 3)):
        out = Buf((C, ld))
        ok(L().dvae_mel_db_normalize(bx.ptr, out.ptr, M, C, ld, col0, ml, rdb, mdb, st()))
        guards(out)
        got, gb = out.np(), out.bits()
        note("mel_db_normalize", got[:, col0:col0 + M], ref, tol, f"M={M} C={C} ld={ld} col0={col0} {pname}")
        untouched(gb[:, :col0], "columns in front of col0")
        untouched(gb[:, col0 + M:], "columns behind col0 + M")
        floor_bits = np.unique(gb[:, col0:col0 + M][(x <= F32(ml)).T])
        assert floor_bits.size == 1, "inputs at and below min_level give more than one value"
    out = Buf((C, M + 1))
    assert L().dvae_mel_db_normalize(bx.ptr, out.ptr, M, C, M + 1, 2, ml, rdb, mdb, st()) == EINVAL   # col0 + M > ld_out
    untouched(out.bits(), "a refused call")


@pytest.mark.parametrize("Ms", [(1, 5, 37), (20, 25, 20), (33,)], ids=["1_5_37", "tile_spans_two", "one"])
def test_mel_db_normalize_seg(Ms):
    rs = np.random.RandomState(sum(Ms))
    ml, rdb, mdb = PARAMS["production"]
    for C in (80, 33):
        rows = sum(Ms)
        seg = A.seg_table(Ms, [0] * len(Ms))
        x = A.db_edge_values(rs, rows, C, ml, rdb, mdb)
        bx, bs, out = Pad(x), ibuf(seg), Buf((C * rows,))
        ok(L().dvae_mel_db_normalize_seg(bx.ptr, out.ptr, bs.ptr, len(Ms), rows, C, ml, rdb, mdb, st()))
        guards(out)
        got = out.np()
        for row0, M, _, _ in seg:
            ref, tol, _ = A.db_normalize_bounds(x[row0:row0 + M], ml, rdb, mdb)
            note("mel_db_normalize_seg", got[C * row0:C * (row0 + M)].reshape(C, M), ref, tol, f"Ms={Ms} C={C} row0={row0}")


@pytest.mark.parametrize("L_,C", A.CASES["transpose"])
def test_mel_denormalize(L_, C):
    rs = np.random.RandomState(L_ * 100 + C + 1)
    rdb, mdb = 16.0, -100.0
    for ld in (L_, L_ + 5):
        mel, core = np.full((C, ld), np.nan, F32), rs.uniform(-0.1, 1.1, (C, L_)).astype(F32)
        core.reshape(-1)[:3] = np.array([0.0, 1.0, A.nextf(1.0, False)], F32)[:C * L_]
        mel[:, :L_] = core
        bm, out = Pad(mel), Buf((L_, C))
        ok(L().dvae_mel_denormalize(bm.ptr, out.ptr, L_, C, ld, rdb, mdb, st()))
        guards(out)
        ref, tol = A.denormalize_bounds(mel[:, :L_], rdb, mdb)
        assert np.isfinite(tol).all()
        note("mel_denormalize", out.np(), ref, tol, f"L={L_} C={C} ld_in={ld}")
        if ld == L_:                                                     # the pair: normalise(denormalise(m)) == clip(m)
            back = Buf((C, L_))
            ok(L().dvae_mel_db_normalize(out.ptr, back.ptr, L_, C, L_, 0, 1e-5, rdb, mdb, st()))
            guards(back)
            bref, btol, _ = A.db_normalize_bounds(out.np(), 1e-5, rdb, mdb)
            note("mel_db_normalize", back.np(), bref, btol, f"after denormalize L={L_} C={C}")
            # the pair: amp is within tol of 10^a with a = db * fl32(0.05), not db / 20: q moves by 20 |a| |20 fl32(0.05) - 1| / 100
            prop = (20 / np.log(10) * tol / ref + 20 * np.abs(np.log10(ref)) * abs(20 * F64(F32(0.05)) - 1)) / 100 * 1.01
            note("mel round trip", back.np(), np.clip(core.astype(F64), 0, 1), btol + prop.T, f"L={L_} C={C}")
    assert L().dvae_mel_denormalize(bm.ptr, out.ptr, L_, C, L_ - 1, rdb, mdb, st()) == EINVAL


# ------------------------------------------------------------------ nnls
def nnls_launch(amp, x, fr, bf, bw, step, iters):
    ba, bx = Pad(amp), Buf(None, data=np.ascontiguousarray(x, F32))
    bfr, bbf, bbw = ibuf(fr, np.int32), ibuf(bf, np.int32), Pad(bw)
    rc = L().dvae_mel_nnls_pg(ba.ptr, bx.ptr, x.shape[0], x.shape[1], amp.shape[1], bfr.ptr, bbf.ptr, bbw.ptr, float(step), iters, st())
    guards(bx)
    return rc, bx


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("nbp,C", [(1, 1), (5, 3), (129, 2), (516, 80), (1024, 128)])
def test_mel_nnls_pg(nbp, C, rows):
    rs = np.random.RandomState(nbp + rows)
    fr, bf, bw, dense = A.mel_tables(nbp, C, rs, integer=True)
    x0, amp = rs.randint(0, 5, (rows, nbp)).astype(F32), rs.randint(0, 9, (rows, C)).astype(F32)
    rc, bx = nnls_launch(amp, x0, fr, bf, bw, 2.0 ** -3, 3)
    ok(rc)
    assert_same_bits(bx, A.nnls_bounds(x0, amp, fr, bf, bw, 2.0 ** -3, 3)[0].astype(F32), f"nnls class E nbp={nbp} C={C}")
    fr, bf, bw, dense = A.mel_tables(nbp, C, rs, integer=False)
    x0, amp = np.abs(A.rfull(rs, (rows, nbp), -4, 2)), np.abs(A.rfull(rs, (rows, C), -4, 2))
    step = F32(0.9 / np.linalg.norm(dense, 2) ** 2)
    rc, bx = nnls_launch(amp, x0, fr, bf, bw, step, 0)
    ok(rc)
    assert_same_bits(bx, x0, "nnls iters = 0 leaves x alone")
    rc, bx = nnls_launch(amp, x0, fr, bf, bw, step, 1)
    ok(rc)
    ref, tol, _ = A.nnls_bounds(x0, amp, fr, bf, bw, step, 1)
    got = bx.np()
    note("mel_nnls_pg one step", got, ref, tol, f"nbp={nbp} C={C}")
    unf = ~dense.any(0)
    assert_same_bits(got[:, unf], x0[:, unf], "a bin under no filter keeps its bits")
    rc, bx = nnls_launch(amp, x0, fr, bf, bw, step, 7)
    ok(rc)
    ref, _, n2 = A.nnls_bounds(x0, amp, fr, bf, bw, step, 7)
    err = np.sqrt(((bx.np().astype(F64) - ref) ** 2).sum(1))
    note("mel_nnls_pg 7 steps, row 2-norm", err, np.zeros(rows), n2, f"nbp={nbp} C={C}")
    assert_same_bits(bx.np()[:, unf], x0[:, unf], "a bin under no filter keeps its bits")


def test_mel_nnls_pg_refusals():
    rs = np.random.RandomState(0)
    fr, bf, bw, _ = A.mel_tables(8, 2, rs, True)
    big = np.zeros((1, 1025), F32)
    assert nnls_launch(np.zeros((1, 2), F32), big, fr, np.full((1025, 2), -1, np.int32), np.zeros((1025, 2), F32), 0.5, 1)[0] == EINVAL
    assert nnls_launch(np.zeros((1, 129), F32), np.zeros((1, 8), F32), np.zeros((129, 2), np.int32), bf, bw, 0.5, 1)[0] == EINVAL
    assert nnls_launch(np.zeros((1, 2), F32), np.zeros((1, 8), F32), fr, bf, bw, 0.0, 1)[0] == EINVAL


# ------------------------------------------------------------------ ola
def test_gl_segment_table():
    for frames, fsize, hop in (([2, 3, 9], 8, 4), ([4, 5, 9], 16, 4), ([1, 2, 9], 8, 8), ([3, 4, 9], 24, 8), ([1, 3], 8, 4),
                               ([3, 4], 20, 8), ([2, 2], 8, 6), ([2], 6, 2), ([2], 8, 16)):
        ref = A.gl_segment_table(frames, fsize, hop)
        tab = np.full((len(frames), 4), -7, np.int64)
        fr = np.array(frames, np.int32)
        rc = L().dvae_gl_segment_table(fr.ctypes.data, len(frames), fsize, hop, tab.ctypes.data)
        if ref is None:
            assert rc == EINVAL
        else:
            ok(rc)
            assert np.array_equal(tab, ref)


@pytest.mark.parametrize("integer", [True, False], ids=["E", "R"])
@pytest.mark.parametrize("fsize,hop", A.CASES["ola"])
def test_ola_gather(fsize, hop, integer):
    rs = np.random.RandomState(fsize + hop)
    k0 = -(-fsize // hop)
    Ms = [k0, k0 + 1, 9]
    for gap in (0, 4):
        segs, rows, win, y = ola_case(rs, fsize, hop, Ms, integer)
        segs = A.seg_table(Ms, segs[:, 3].tolist(), gap)
        out_len = int(segs[-1][2] + segs[-1][3] + gap)
        by, bw, bs = Pad(y), Pad(win), ibuf(segs)
        for mode in (0, 1):
            for norm in (0, 1):
                out = Buf((rows, fsize) if mode == 0 else (out_len,))
                ok(L().dvae_ola_gather(by.ptr, bs.ptr, len(Ms), rows, bw.ptr, out.ptr, out_len, fsize, hop, mode, norm, st()))
                guards(out)
                ref, tol = A.ola_bounds(y, win, segs, rows, out_len, fsize, hop, mode, norm)
                what = f"ola {fsize}/{hop} mode={mode} norm={norm} gap={gap}"
                if integer:
                    assert_same_bits(out, ref.astype(F32), what + " class E")
                else:
                    note(f"ola_gather mode {mode}" + (" norm" if norm else ""), out.np(), ref, tol, what)
                    assert not out.bits()[ref == 0].any() or mode == 0, what + ": a gap is not +0"


def test_ola_gather_envelope_branch_and_refusals():
    rs = np.random.RandomState(9)
    segs, rows, win, y = ola_case(rs, 8, 8, [1, 2, 9], False)
    win[2] = win[5] = 0.0
    out_len = int(segs[-1][2] + segs[-1][3])
    by, bw, bs, out = Pad(y), Pad(win), ibuf(segs), Buf((out_len,))
    ok(L().dvae_ola_gather(by.ptr, bs.ptr, 3, rows, bw.ptr, out.ptr, out_len, 8, 8, 1, 1, st()))
    guards(out)
    ref, tol = A.ola_bounds(y, win, segs, rows, out_len, 8, 8, 1, 1)
    note("ola_gather mode 1 norm", out.np(), ref, tol, "envelope branch")
    assert not out.bits()[2::8].any() and not out.bits()[5::8].any(), "e <= 1e-20 must give +0"
    for args in ((out_len, 8, 6, 1), (out_len, 6, 2, 1), (out_len + 2, 8, 8, 1), (out_len, 8, 16, 1), (out_len, 8, 8, 2)):
        assert L().dvae_ola_gather(by.ptr, bs.ptr, 3, rows, bw.ptr, out.ptr, args[0], args[1], args[2], args[3], 0, st()) == EINVAL
    assert L().dvae_ola_gather(by.ptr + 4, bs.ptr, 3, rows, bw.ptr, out.ptr, out_len, 8, 8, 1, 0, st()) == EINVAL


# ------------------------------------------------------------------ resample
def resample_tables_dev(n_in, filt, filters, tile):
    """the entry point's own table and tiles, checked against the restatement"""
    n_in, filt = np.array(n_in, np.int64), np.array(filt, np.int32)
    table = np.full((len(n_in), 6), -7, np.int64)
    fl = np.ascontiguousarray(filters, np.int64)
    nt = L().dvae_resample_segment_table(n_in.ctypes.data, filt.ctypes.data, len(n_in), fl.ctypes.data, len(fl), tile,
                                         table.ctypes.data, None, 0)
    ref = A.resample_segment_table(n_in.tolist(), filt.tolist(), filters, tile)
    if ref is None:
        assert nt == EINVAL
        return None
    assert nt == len(ref[1])
    tiles = np.full((nt, 2), -7, np.int64)
    assert L().dvae_resample_segment_table(n_in.ctypes.data, filt.ctypes.data, len(n_in), fl.ctypes.data, len(fl), tile,
                                           table.ctypes.data, tiles.ctypes.data, nt) == nt
    assert np.array_equal(table, ref[0]) and np.array_equal(tiles, ref[1])
    if nt > 1:
        assert L().dvae_resample_segment_table(n_in.ctypes.data, filt.ctypes.data, len(n_in), fl.ctypes.data, len(fl), tile,
                                               table.ctypes.data, tiles.ctypes.data, nt - 1) == EINVAL
    return table, tiles


def resample_run(filters, weights, table, tiles, x, what, integer):
    lds = max(L().dvae_resample_lds_floats(int(P), int(Q), int(tp)) for P, Q, tp in filters[:, :3])
    assert lds == max(A.resample_lds_floats(int(P), int(Q), int(tp)) for P, Q, tp in filters[:, :3])
    A.resample_geometry(table, filters, lds)
    total = int(table[-1][2] + (table[-1][3] + 3) // 4 * 4)
    bx, bw, y = Pad(x), Pad(weights), Buf((total,))
    bt, bf, bl = ibuf(table), ibuf(filters), ibuf(tiles)
    ok(L().dvae_resample_batch(bx.ptr, y.ptr, bt.ptr, bf.ptr, bw.ptr, bl.ptr, len(tiles), lds, st()))
    guards(y)
    ref, tol, written = A.resample_bounds(np.nan_to_num(x), table, filters, weights)
    got, gb = y.np(), y.bits()
    assert np.isfinite(got[written]).all(), what + ": the NaN sentinel (or an unwritten output) inside a segment"
    untouched(gb[~written], what + " between the segments")
    if integer:
        assert_same_bits(got[written], ref[written].astype(F32), what + " class E")
    else:
        note("resample_batch", got[written], ref[written], tol[written], what)
    for in0, n, out0, n_out, nv, f in table:
        assert not gb[out0 + nv:out0 + n_out].any(), what + ": the tail n_valid <= t < n_out is not +0"
    return bx, bw, y, bt, bf, bl, lds


@pytest.mark.parametrize("integer", [True, False], ids=["E", "R"])
@pytest.mark.parametrize("n_valid", A.CASES["resample_n_valid"])
def test_resample_batch_hand_filters(n_valid, integer):
    rs = np.random.RandomState(10 + n_valid)
    filters, weights = A.resample_hand_filters(rs, integer)
    n_in = [A.n_in_for_valid(n_valid, int(P), int(Q)) + (i % 2) for i, (P, Q) in enumerate(filters[:, :2])]
    table, tiles = resample_tables_dev(n_in, list(range(len(filters))), filters, A.RS_TILE)
    assert (table[::2, 4] == n_valid).all()
    shift = np.cumsum([0, 0, 1, 0, 2, 0, 1])                             # hand-built starts that are not 16-byte aligned
    table = table.copy()
    table[:, 0] += shift + 0 * 4
    x = np.full(int(table[-1][0] + table[-1][1] + 8), np.nan, F32)
    for in0, n, *_ in table:
        x[in0:in0 + n] = rs.randint(-4, 5, n) if integer else A.rfull(rs, (n,), -3, 3)
    geo = A.resample_geometry(table, filters, 1 << 14)
    assert geo["g0_negative"] >= 1 and geo["unaligned"] >= 1 and geo["edge_loads"] >= 1
    resample_run(filters, weights, table, tiles, x, f"resample n_valid={n_valid}", integer)


@pytest.mark.parametrize("sr", [48000, 44100])
def test_resample_batch_real_filter_and_refusals(sr):
    from dvae_amd.preprocess import resample_filter
    rs = np.random.RandomState(sr)
    t = resample_filter(sr)
    filters = np.array([[t["P"], t["Q"], t["taps"], t["base"], 0, 0]], np.int64)
    weights = t["weights"].astype(F32).reshape(-1)
    table, tiles = resample_tables_dev([601, 7 * t["Q"] // t["P"] + 1], [0, 0], filters, A.RS_TILE)
    x = np.full(int(table[-1][0] + table[-1][1] + 4), np.nan, F32)
    for in0, n, *_ in table:
        x[in0:in0 + n] = A.rfull(rs, (n,), -3, 0)
    bx, bw, y, bt, bf, bl, lds = resample_run(filters, weights, table, tiles, x, f"resample_filter({sr})", False)
    args = lambda **k: [k.get("x", bx.ptr), k.get("y", y.ptr), bt.ptr, bf.ptr, bw.ptr, bl.ptr, len(tiles), k.get("lds", lds), st()]  # noqa: E731
    before = y.bits()
    for bad in (dict(x=bx.ptr + 4), dict(y=y.ptr + 8), dict(lds=lds + 2), dict(lds=16388), dict(lds=0)):
        assert L().dvae_resample_batch(*args(**bad)) == EINVAL, bad
    assert np.array_equal(y.bits(), before)
    assert L().dvae_resample_lds_floats(1, 64, 16) == 16344 and L().dvae_resample_lds_floats(1, 65, 16) == EINVAL
    assert L().dvae_resample_lds_floats(0, 1, 1) == EINVAL
    assert resample_tables_dev([600, 2], [0, 1], np.array([[160, 441, 9, 4, 0, 0], [1, 3, 4, 2, 0, 0]]), 256) is None
    assert resample_tables_dev([600], [1], filters, 256) is None


# ------------------------------------------------------------------ volume
@pytest.mark.parametrize("increase_only", [0, 1])
def test_volume_normalize(increase_only):
    rs = np.random.RandomState(11)
    n_outs = [1, 7, 2047, 2048, 2049, 4100, 5, 3]
    segs, tiles, first = A.volume_table(n_outs)
    y = np.full(int(segs[-1][2] + 4), np.nan, F32)
    for s, (_, n, out0, *_r) in enumerate(segs):
        y[out0:out0 + n] = 0.0 if s == 1 else A.rfull(rs, (n,), -12, -4) * (1000.0 if s in (2, 7) else 1.0)
    by = Buf(None, data=y)
    part, ms, gain, silent = Buf((len(tiles),), torch.float64), Buf((len(n_outs),), torch.float64), Buf((len(n_outs),)), \
        Buf((len(n_outs),), torch.int32)
    bs, bt, bf = ibuf(segs), ibuf(tiles), ibuf(first)
    ok(L().dvae_volume_normalize(by.ptr, bs.ptr, len(n_outs), bt.ptr, len(tiles), bf.ptr, part.ptr, -30.0, increase_only, ms.ptr,
                                 gain.ptr, silent.ptr, st()))
    guards(by, part, ms, gain, silent)
    b = A.volume_bounds(np.nan_to_num(y), segs, tiles, first, -30.0, increase_only)
    assert np.array_equal(part.bits(), b["part"].view(np.int64)), "part is not the documented order's float64 sum"
    note("volume part", part.np(), b["part_sum"], b["tol_part"] + A.FLOOR, "against the exact sum")
    note("volume ms", ms.np(), b["ms_true"], b["tol_ms"] + A.FLOOR, "ms_out")
    note("volume gain", gain.np(), b["gain"], b["tol_gain"] + A.FLOOR, f"increase_only={increase_only}")
    assert np.array_equal(silent.np(), b["silent"])
    gd, got = gain.np(), by.np()
    assert gd[1] == 1.0 and (gd[2] == 1.0) == bool(increase_only) and (gd[7] == 1.0) == bool(increase_only)
    for s, (_, n, out0, *_r) in enumerate(segs):
        assert_same_bits(got[out0:out0 + n], y[out0:out0 + n] * F32(gd[s]), f"volume segment {s}: y * the device's own gain")
    assert np.isnan(got[np.isnan(y)]).all()
    assert L().dvae_volume_normalize(by.ptr, bs.ptr, len(n_outs), bt.ptr, len(tiles), bf.ptr, part.ptr, 2000.0, 0, ms.ptr, gain.ptr,
                                     silent.ptr, st()) == EINVAL


# ------------------------------------------------------------------ log_power
@pytest.mark.parametrize("rows,nb,nbp", A.CASES["log_power"])
def test_log_power(rows, nb, nbp):
    rs = np.random.RandomState(rows + nb)
    floor = 2.0 ** -20
    x = log_power_case(rs, rows, nb, nbp, floor)
    bx, pw, lp = Pad(x), Buf((rows, nbp)), Buf((rows, nbp))
    ok(L().dvae_log_power(bx.ptr, pw.ptr, lp.ptr, rows, nb, nbp, floor, st()))
    guards(pw, lp)
    p, tp, l, tl, below = A.log_power_bounds(np.nan_to_num(x), nb, nbp, floor)
    note("log_power power", pw.np(), p, tp, f"rows={rows} nb={nb}")
    note("log_power log", lp.np(), l, tl, f"rows={rows} nb={nb}")
    assert not pw.bits()[:, nb:].any() and not lp.bits()[:, nb:].any(), "bins nb..nbp are not +0"
    assert np.unique(lp.bits()[below]).size <= 1, "more than one value below the floor"
    e = np.zeros((rows, 2 * nbp), F32)                                   # class E: 2^a, 2^a -> power 2^(2a+1) exactly
    sc = (2.0 ** rs.randint(-3, 4, (rows, nbp))).astype(F32)
    e[:, :nbp], e[:, nbp:] = sc, -sc
    be, pe, le = Pad(e), Buf((rows, nbp)), Buf((rows, nbp))
    ok(L().dvae_log_power(be.ptr, pe.ptr, le.ptr, rows, nb, nbp, floor, st()))
    guards(pe, le)
    want = 2 * sc * sc
    want[:, nb:] = 0
    assert_same_bits(pe, want, "log_power class E")
    assert L().dvae_log_power(be.ptr, pe.ptr, le.ptr, rows, nbp + 1, nbp, floor, st()) == EINVAL


# ------------------------------------------------------------------ voicing
def voicing_launch(r, ldr, nlag, gain, mc, ldm, segs, peak_min, rel_min):
    rows = r.shape[0]
    br, bg, bm, bs = Pad(r), Pad(gain), Pad(mc), ibuf(segs)
    peak, voiced, feats, count = Buf((rows,)), Buf((rows,), torch.int32), Buf((rows, 24)), Buf((len(segs),), torch.int32)
    ok(L().dvae_voicing_compact(br.ptr, ldr, nlag, bg.ptr, bm.ptr, ldm, bs.ptr, len(segs), peak_min, rel_min, peak.ptr, voiced.ptr,
                                feats.ptr, count.ptr, st()))
    guards(peak, voiced, feats, count)
    return peak, voiced, feats, count


def check_voicing_exact(b, peak, voiced, feats, count, what):
    assert_same_bits(peak, b["peak"].astype(F32), what + " peak")
    assert np.array_equal(voiced.np(), b["voiced"]), what + " voiced"
    assert np.array_equal(count.np(), b["count"]), what + " count"
    fb, wr = feats.bits(), ~np.isnan(b["feats"][:, 0])
    assert_same_bits(feats.np()[wr], b["feats"][wr], what + " feats")
    untouched(fb[~wr], what + " feats beyond row0 + count")


@pytest.mark.parametrize("pattern", ["all", "none", "alt", "last_of_chunk", "first_of_next", "edges"])
@pytest.mark.parametrize("M", A.CASES["voicing_M"])
def test_voicing_compact_class_e(M, pattern):
    nlag = A.CASES["voicing_nlag"][(M + len(pattern)) % 5]
    r, gain, mc = A.voicing_e_case(M, nlag, pattern, M, ldr=nlag + 3, ldm=28)
    segs = A.seg_table([M], [0])
    out = voicing_launch(r, nlag + 3, nlag, gain, mc, 28, segs, 0.5, 2.0 ** -4)
    b = A.voicing_bounds(np.nan_to_num(r), nlag, np.nan_to_num(gain), mc, segs, 0.5, 2.0 ** -4)
    check_voicing_exact(b, *out, f"voicing E M={M} nlag={nlag} {pattern}")


@pytest.mark.parametrize("nlag", A.CASES["voicing_nlag"])
def test_voicing_compact_three_utterances(nlag):
    Ms, pats = (65, 256, 130), ("alt", "all", "edges")
    parts = [A.voicing_e_case(M, nlag, p, 7 + i, ldr=nlag + 1, ldm=24) for i, (M, p) in enumerate(zip(Ms, pats))]
    gain = parts[0][1]
    assert all(np.array_equal(q[1], gain, equal_nan=True) for q in parts)
    r, mc = np.concatenate([q[0] for q in parts]), np.concatenate([q[2] for q in parts])
    segs = A.seg_table(Ms, [0, 0, 0])
    out = voicing_launch(r, nlag + 1, nlag, gain, mc, 24, segs, 0.5, 2.0 ** -4)
    b = A.voicing_bounds(r, nlag, np.nan_to_num(gain), mc, segs, 0.5, 2.0 ** -4)
    check_voicing_exact(b, *out, f"voicing E three utterances nlag={nlag}")


@pytest.mark.parametrize("M", A.CASES["voicing_M"])
def test_voicing_compact_class_r(M):
    rs = np.random.RandomState(13 + M)
    for nlag in (1, 65, 206):
        r, gain, mc = voicing_r_case(rs, M, nlag)
        segs = A.seg_table([M], [0])
        peak, voiced, feats, count = voicing_launch(r, nlag + 1, nlag, gain, mc, 24, segs, 0.45, 0.01)
        b = A.voicing_bounds(r, nlag, gain, mc, segs, 0.45, 0.01)
        note("voicing peak", peak.np(), b["peak"], b["tol_peak"], f"M={M} nlag={nlag}")
        dec = b["decided"]
        assert (~dec).sum() <= 0.01 * M
        v = voiced.np()
        assert np.array_equal(v[dec], b["voiced"][dec]), f"voicing R M={M} nlag={nlag}: a decided flag differs"
        assert count.np()[0] == v.sum()
        assert_same_bits(feats.np()[:v.sum()], mc[v.astype(bool), :24], "feats: the voiced rows in time order")
        untouched(feats.bits()[v.sum():], "feats beyond count")


# ------------------------------------------------------------------ DTW
def dtw_launch(x, y, lx=None, ly=None):
    """one launch over the pairs (x, y) and (y, x): both swap paths"""
    nx, ny = len(x), len(y)
    X, Y = np.concatenate([x, y]).astype(F32).reshape(-1, 24), np.concatenate([y, x]).astype(F32).reshape(-1, 24)
    pairs = np.array([[0, nx, 0, ny], [nx, ny, ny, nx]], np.int64)
    bx, by, bp = Pad(X), Pad(Y), ibuf(pairs)
    cost, length = Buf((2,), torch.float64), Buf((2,), I64)
    ok(L().dvae_dtw_batch(bx.ptr, by.ptr, bp.ptr, pairs.ctypes.data, 2, cost.ptr, length.ptr, st()))
    guards(cost, length)
    sse = None
    if lx is not None:
        blx, bly = Pad(np.concatenate([lx, ly])), Pad(np.concatenate([ly, lx]))
        c2, l2, sse = Buf((2,), torch.float64), Buf((2,), I64), Buf((2,), torch.float64)
        ok(L().dvae_dtw_batch_f0(bx.ptr, by.ptr, blx.ptr, bly.ptr, bp.ptr, pairs.ctypes.data, 2, c2.ptr, l2.ptr, sse.ptr, st()))
        guards(c2, l2, sse)
        assert np.array_equal(c2.bits(), cost.bits()) and np.array_equal(l2.np(), length.np()), "the payload changed cost or length"
        sse = sse.np()
    return cost.np(), length.np(), sse


@pytest.mark.parametrize("nx,ny", A.CASES["dtw_r"])
def test_dtw_batch_class_r(nx, ny):
    x, y, lx, ly = dtw_r_case(nx, ny)
    cost, length, sse = dtw_launch(x, y, lx, ly)
    for p, d in enumerate((A.dtw_full(x, y, lx, ly), A.dtw_full(y, x, ly, lx))):
        assert d["margin_ok"]
        what = f"dtw {nx}x{ny} pair {p}"
        note("dtw cost", cost[p], d["cost"], d["bound"], what)
        assert length[p] == d["length"], what + f": length {length[p]} instead of {d['length']}"
        note("dtw_f0 sse", sse[p], d["sse"], d["tol_sse"], what)


@pytest.mark.parametrize("name", list(A.dtw_e_cases()))
def test_dtw_batch_class_e(name):
    x, y, want = A.dtw_e_cases()[name]
    lx, ly = np.arange(len(x), dtype=F32) % 5, np.arange(len(y), dtype=F32) % 3
    cost, length, sse = dtw_launch(x, y, lx, ly)
    for p, d in enumerate((A.dtw_full(x, y, lx, ly), A.dtw_full(y, x, ly, lx))):
        assert cost[p] == d["cost"] and length[p] == d["length"], f"{name} pair {p}: ({cost[p]}, {length[p]}) instead of " \
                                                                  f"({d['cost']}, {d['length']})"
        assert sse[p] == d["sse"], f"{name}: integer payload"
    if want is not None:
        assert length[0] == want and length[1] == want


def test_dtw_batch_empty_side_and_refusals():
    x, y, lx, ly = dtw_r_case(3, 4)
    bx, by, blx, bly = Pad(x), Pad(y), Pad(lx), Pad(ly)
    pairs = np.array([[0, 0, 0, 4], [0, 3, 0, 0], [0, 3, 0, 4], [0, 0, 0, 0]], np.int64)
    bp = ibuf(pairs)
    cost, length, sse = Buf((4,), torch.float64), Buf((4,), I64), Buf((4,), torch.float64)
    ok(L().dvae_dtw_batch_f0(bx.ptr, by.ptr, blx.ptr, bly.ptr, bp.ptr, pairs.ctypes.data, 4, cost.ptr, length.ptr, sse.ptr, st()))
    guards(cost, length, sse)
    c, l, s = cost.np(), length.np(), sse.np()
    assert np.isnan(c[[0, 1, 3]]).all() and np.isnan(s[[0, 1, 3]]).all() and not l[[0, 1, 3]].any()
    d = A.dtw_full(x, y, lx, ly)
    assert abs(c[2] - d["cost"]) <= d["bound"] and l[2] == d["length"]
    for bad in ([[0, 4097, 0, 4097]], [[0, -1, 0, 4]], [[-1, 3, 0, 4]], [[0, 3, 0, (1 << 30) + 1]]):
        ph = np.array(bad, np.int64)
        c2 = Buf((1,), torch.float64)
        assert L().dvae_dtw_batch(bx.ptr, by.ptr, bp.ptr, ph.ctypes.data, 1, c2.ptr, length.ptr, st()) == EINVAL
        untouched(c2.bits(), "a refused DTW")
    assert L().dvae_dtw_batch(bx.ptr + 4, by.ptr, bp.ptr, pairs.ctypes.data, 4, cost.ptr, length.ptr, st()) == EINVAL


# ------------------------------------------------------------------ F0 Viterbi
@pytest.mark.parametrize("jump", [0.5, 0.0])
def test_f0_viterbi_class_e(jump):
    r, gain, v, segs = A.viterbi_e_case()
    l2, oc = A.viterbi_tables()
    rows = r.shape[0]
    br, bg, bv, bs = Pad(r), Pad(gain), ibuf(v, np.int32), ibuf(segs)
    bl2, boc = Buf(None, data=l2), Buf(None, data=oc)
    back, lag, f0, lf = Buf((rows, A.F0_BACK_LD), torch.uint8), Buf((rows,), torch.int32), Buf((rows,)), Buf((rows,))
    ok(L().dvae_f0_viterbi(br.ptr, r.shape[1], A.F0_STATES, bg.ptr, bv.ptr, bs.ptr, len(segs), bl2.ptr, boc.ptr, jump, 16000.0, 20,
                           back.ptr, lag.ptr, f0.ptr, lf.ptr, st()))
    guards(back, lag, f0, lf)
    b = A.viterbi_ref(np.nan_to_num(r), np.nan_to_num(gain), v, segs, l2, oc, jump, 16000.0, 20)
    bad = np.nonzero(lag.np() != b["lag"])[0]
    assert not bad.size, f"lag differs on {bad.size} frames, first at row {bad[:1]}: {lag.np()[bad[:1]]} instead of {b['lag'][bad[:1]]}"
    note("f0_viterbi f0", f0.np(), b["f0"], b["tol_f0"], f"jump={jump}")
    wr = ~np.isnan(b["lf0v"])
    note("f0_viterbi lf0v", lf.np()[wr], b["lf0v"][wr], b["tol_lf0v"][wr], f"jump={jump}")
    untouched(lf.bits()[~wr], "lf0v past the voiced count (an utterance without a voiced frame included)")
    assert not f0.bits()[v == 0].any(), "f0 of an unvoiced frame is not +0"
    assert L().dvae_f0_viterbi(br.ptr, r.shape[1], 205, bg.ptr, bv.ptr, bs.ptr, len(segs), bl2.ptr, boc.ptr, jump, 16000.0, 20,
                               back.ptr, lag.ptr, f0.ptr, lf.ptr, st()) == EINVAL
