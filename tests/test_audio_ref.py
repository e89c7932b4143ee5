"""tests/audio_ref.py on the CPU: every restatement against an independent float64 form, every bound against an fp32 numpy
restatement of the kernel's written order (fused and unfused, the device functions pushed to their constants: the error
stays within the bound and somewhere reaches a stated fraction of it), seeded wrong restatements that must break the bound
or the bits on the named cases, and the launch geometry each named case reaches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as A  # noqa: E402

F32, F64 = np.float32, np.float64


def ratio(got, ref, tol):
    return A.worst_ratio(got, ref, tol)[0]


def held_and_tight(ratios, frac, what):
    assert max(ratios) <= 1.0, f"{what}: an fp32 evaluation of the written order leaves the bound: {ratios}"
    assert max(ratios) >= frac, f"{what}: the bound is vacuous, the worst fp32 evaluation reaches {max(ratios):.3f} of it"


# ------------------------------------------------------------------ frames
def test_frames_restatement_is_the_strided_view_and_an_off_by_one_window_shows():
    rs = np.random.RandomState(0)
    for fsize, hop, left, n in A.CASES["frames"]:
        M = A.frames_count(n, fsize, hop, left)
        wav, win = rs.randint(-8, 9, n).astype(F32), 2.0 ** rs.randint(-2, 3, fsize).astype(F32)
        seg = A.seg_table([M], [n])
        ref = A.frames_ref(wav, win, seg, M, fsize, hop, left)
        padded = np.concatenate([np.zeros(left, F32), wav, np.zeros(M * hop + fsize, F32)])
        ind = np.stack([padded[m * hop:m * hop + fsize] * win for m in range(M)])
        assert np.array_equal(ref, ind)
        assert not ref[-1].any()                                         # the all-padding row
        if n >= 3:
            assert not np.array_equal(ref, A.frames_ref(wav, win, seg, M, fsize, hop, left, win_shift=1))


def test_segmented_frames_are_the_utterances_one_by_one():
    rs = np.random.RandomState(1)
    for fsize, hop, left, ns in A.CASES["frames_seg"]:
        Ms = [A.frames_count(n, fsize, hop, left) for n in ns]
        seg = A.seg_table(Ms, ns)
        wav, win = A.rfull(rs, (sum(ns),)), A.rfull(rs, (fsize,))
        ref = A.frames_ref(wav, win, seg, sum(Ms), fsize, hop, left)
        for (row0, M, s0, n) in seg:
            one = A.frames_ref(wav[s0:s0 + n], win, A.seg_table([M], [n]), M, fsize, hop, left)
            assert np.array_equal(ref[row0:row0 + M], one)


# ------------------------------------------------------------------ magnitude, gl_init, gl_phase
def reim_case(rs, rows, nbp):
    return A.rfull(rs, (rows, 2 * nbp))


def test_magnitude_bound_holds_for_every_fp32_evaluation_and_is_not_vacuous():
    rs = np.random.RandomState(2)
    ratios = []
    for rows, nbp in A.CASES["rows_nbp"] + [(64, 516)]:
        x = reim_case(rs, rows, nbp)
        ref, tol = A.magnitude_bounds(x, nbp)
        assert np.allclose(ref, np.abs(x[:, :nbp].astype(F64) + 1j * x[:, nbp:].astype(F64)), rtol=1e-15)
        ratios += [ratio(A.magnitude_f32(x, nbp, fma, push), ref, tol) for fma in (0, 1) for push in (-1, 0, 1)]
    held_and_tight(ratios, 0.5, "stft_magnitude")


def test_gl_init_exact_without_phase_bounded_with_and_a_swapped_block_shows():
    rs = np.random.RandomState(3)
    for rows, nbp in A.CASES["rows_nbp"]:
        mag, ph = np.abs(A.rfull(rs, (rows, nbp))), rs.uniform(-64, 64, (rows, nbp)).astype(F32)
        ref, tol = A.gl_init_bounds(mag, None)
        assert (tol == A.FLOOR).all() and np.array_equal(ref[:, :nbp], mag) and not ref[:, nbp:].any()
        ref, tol = A.gl_init_bounds(mag, ph)
        z = mag.astype(F64) * np.exp(1j * ph.astype(F64))
        assert np.allclose(ref, np.concatenate([z.real, z.imag], 1), rtol=1e-14, atol=1e-300)
        got = np.concatenate([(mag * np.cos(ph.astype(F64)).astype(F32)), (mag * np.sin(ph.astype(F64)).astype(F32))], 1)
        assert ratio(got, ref, tol) <= 1.0
        if rows * nbp > 4:
            assert ratio(got, *A.gl_init_bounds(mag, ph, swap=True)) > 1.0


def gl_phase_case(rs, rows, nbp):
    """class R with the edges: exact zeros of a (both operands 0; rebuilt == alpha prev with prev a power of two), mag 0"""
    reb, prev, mag = reim_case(rs, rows, nbp), reim_case(rs, rows, nbp), np.abs(A.rfull(rs, (rows, nbp)))
    al = A.gl_alpha(0.99)
    flat = rs.permutation(rows * nbp)
    for n_, idx in enumerate(flat[:max(1, rows * nbp // 8)]):
        r, j = divmod(int(idx), nbp)
        if n_ % 2:
            reb[r, j] = reb[r, nbp + j] = prev[r, j] = prev[r, nbp + j] = 0.0
        else:
            prev[r, j], prev[r, nbp + j] = 4.0, -0.5
            reb[r, j], reb[r, nbp + j] = F32(al * F32(4.0)), F32(al * F32(-0.5))
    return reb, prev, mag


def test_gl_phase_bound_exact_zero_branch_and_seeded_zero_branch():
    rs = np.random.RandomState(4)
    ratios = []
    for rows, nbp in A.CASES["rows_nbp"]:
        reb, prev, mag = gl_phase_case(rs, rows, nbp)
        for pv, mom in ((prev, 0.99), (None, 0.99), (prev, 0.0)):
            ref, tol, zero = A.gl_phase_bounds(reb, pv, mag, nbp, mom)
            a = reb.astype(F64) - (0 if pv is None else F64(A.gl_alpha(mom)) * pv.astype(F64))
            z = a[:, :nbp] + 1j * a[:, nbp:]
            with np.errstate(invalid="ignore", divide="ignore"):
                ind = np.where(np.abs(z) > 0, mag * z / np.abs(z), mag)
            assert np.allclose(ref, np.concatenate([ind.real, ind.imag], 1), rtol=1e-13, atol=1e-300)
            for fma in (0, 1):
                got = A.gl_phase_f32(reb, pv, mag, nbp, mom, fma)
                ratios.append(ratio(got, ref, tol))
                assert np.array_equal(got[zero], ref[zero].astype(F32)), "the exact zeros are exact in fp32 too"
            if pv is not None and mom > 0:
                assert zero.any()
                bad, _, _ = A.gl_phase_bounds(reb, pv, mag, nbp, mom, zero_branch=0.0)
                assert ratio(got, bad, tol) > 1.0, "a (0, 0) zero branch goes unnoticed"
        assert np.isfinite(tol).mean() > 0.99
    held_and_tight(ratios, 0.3, "gl_phase")


# ------------------------------------------------------------------ the dB pair
PARAMS = {"production": (1e-5, 20.0, -100.0), "floor_inside": (2.0 ** -6, -10.0, -64.0)}


@pytest.mark.parametrize("pname", list(PARAMS))
def test_db_normalize_bound_clips_floor_and_natural_log(pname):
    rs = np.random.RandomState(5)
    ml, rdb, mdb = PARAMS[pname]
    ratios = []
    for M, C in A.CASES["transpose"]:
        x = A.db_edge_values(rs, M, C, ml, rdb, mdb)
        ref, tol, q = A.db_normalize_bounds(x, ml, rdb, mdb)
        S = 20 * np.log10(np.maximum(x.astype(F64), F64(F32(ml)))) - rdb
        assert np.allclose(ref, np.clip((S - mdb) / -mdb, 0, 1).T, atol=1e-12)
        ratios += [ratio(A.db_normalize_f32(x, ml, rdb, mdb, fma, push), ref, tol) for fma in (0, 1) for push in (-1, 0, 1)]
        if M * C > 100:
            assert (tol == A.FLOOR).any() or pname == "floor_inside"
            bad, _, _ = A.db_normalize_bounds(x, ml, rdb, mdb, log=np.log)
            assert ratio(A.db_normalize_f32(x, ml, rdb, mdb, 0), bad, tol) > 1.0, "a natural logarithm goes unnoticed"
    held_and_tight(ratios, 0.25, "mel_db_normalize")


def test_denormalize_bound_and_round_trip():
    rs = np.random.RandomState(6)
    rdb, mdb = 16.0, -100.0                                              # the exponent spans exactly the swept [-4.2, 0.8]
    ratios = []
    for L, C in A.CASES["transpose"]:
        mel = rs.uniform(-0.1, 1.1, (C, L)).astype(F32)
        mel.reshape(-1)[:3] = np.array([0.0, 1.0, A.nextf(1.0, False)], F32)[:mel.size]
        ref, tol = A.denormalize_bounds(mel, rdb, mdb)
        assert np.isfinite(tol).all()
        assert np.allclose(ref, 10 ** ((np.clip(mel.astype(F64), 0, 1) * 100 - 100 + 16) * F64(F32(0.05))).T, rtol=1e-12)
        ratios += [ratio(A.denormalize_f32(mel, rdb, mdb, fma, push), ref, tol) for fma in (0, 1) for push in (-1, 0, 1)]
        back, tb, _ = A.db_normalize_bounds(ref, 1e-5, rdb, mdb)         # the pair: normalise(denormalise(m)) = clip(m)
        assert np.allclose(back, np.clip(mel, 0, 1), atol=1e-6)
    held_and_tight(ratios, 0.25, "mel_denormalize")
    _, tol = A.denormalize_bounds(np.ones((1, 1), F32), 20.0, -100.0)    # production: exponent 1.0, outside the sweep
    assert np.isinf(tol).all()


# ------------------------------------------------------------------ nnls
@pytest.mark.parametrize("nbp,C", [(1, 1), (5, 3), (129, 2), (516, 80)])
def test_nnls_tables_dense_form_class_e_and_bounds(nbp, C):
    rs = np.random.RandomState(7)
    fr, bf, bw, dense = A.mel_tables(nbp, C, rs, integer=True)
    x0 = rs.randint(0, 5, (3, nbp)).astype(F32)
    amp = rs.randint(0, 9, (3, C)).astype(F32)
    step = 2.0 ** -3
    x64 = x0.astype(F64)
    for _ in range(3):                                                   # the dense form, bins under no filter untouched
        x64 = np.where(dense.any(0)[None, :], np.maximum(0, x64 - step * (x64 @ dense.T - amp) @ dense), x64)
    ref, _, _ = A.nnls_bounds(x0, amp, fr, bf, bw, step, 3)
    assert np.array_equal(ref, x64)
    for fma in (0, 1):                                                   # class E: exact whatever is fused
        assert np.array_equal(A.nnls_f32(x0, amp, fr, bf, bw, step, 3, fma).astype(F64), ref)
    fr, bf, bw, dense = A.mel_tables(nbp, C, rs, integer=False)
    x0, amp = np.abs(A.rfull(rs, (3, nbp), -4, 2)), np.abs(A.rfull(rs, (3, C), -4, 2))
    step = F32(0.9 / np.linalg.norm(dense, 2) ** 2)
    ref1, tol1, _ = A.nnls_bounds(x0, amp, fr, bf, bw, step, 1)
    ratios = [ratio(A.nnls_f32(x0, amp, fr, bf, bw, step, 1, fma), ref1, tol1) for fma in (0, 1)]
    assert max(ratios) <= 1.0 and (max(ratios) >= 0.05 or nbp == 1)
    ref7, _, n2 = A.nnls_bounds(x0, amp, fr, bf, bw, step, 7)
    for fma in (0, 1):
        err = np.sqrt(((A.nnls_f32(x0, amp, fr, bf, bw, step, 7, fma).astype(F64) - ref7) ** 2).sum(1))
        assert (err <= n2).all()
    unf = ~dense.any(0)
    assert np.array_equal(ref7[:, unf], x0[:, unf].astype(F64))


# ------------------------------------------------------------------ ola
def ola_case(rs, fsize, hop, Ms, integer, zero_window=False):
    left = fsize - hop
    segs = A.seg_table(Ms, [M * hop - left for M in Ms])
    rows = sum(Ms)
    if integer:                                                          # envelope a power of two: w = 2^k constant
        win, y = np.full(fsize, 2.0, F32), rs.randint(-4, 5, (rows, fsize)).astype(F32)
        if -(-fsize // hop) == 3:
            win[2 * hop:] = 0.0                                          # two frames of weight 4 everywhere: e = 8
    else:
        win, y = (0.1 + rs.rand(fsize)).astype(F32), A.rfull(rs, (rows, fsize), -3, 3)
    if zero_window:
        win[:: 2] = 0.0 if fsize % hop == 0 and hop % 2 == 0 else win[:: 2]
    return segs, rows, win, y


@pytest.mark.parametrize("fsize,hop", A.CASES["ola"])
def test_ola_restatement_bounds_and_seeded_mistakes(fsize, hop):
    rs = np.random.RandomState(8)
    k0 = -(-fsize // hop)
    Ms = [k0, k0 + 1, 9]
    left = fsize - hop
    if fsize % hop == 0:
        assert np.array_equal(A.seg_table(Ms, [M * hop - left for M in Ms]), A.gl_segment_table(Ms, fsize, hop))
    else:
        assert A.gl_segment_table(Ms, fsize, hop) is None
    ratios = []
    for integer in (True, False):
        segs, rows, win, y = ola_case(rs, fsize, hop, Ms, integer)
        out_len = int(segs[-1][2] + segs[-1][3])
        for mode in (0, 1):
            for norm in (0, 1):
                ref, tol = A.ola_bounds(y, win, segs, rows, out_len, fsize, hop, mode, norm)
                if mode == 1:                                            # independent: a padded buffer, frame by frame
                    for row0, M, s0, n in segs:
                        buf, env = np.zeros(M * hop + fsize), np.zeros(M * hop + fsize)
                        for m in range(M):
                            buf[m * hop:m * hop + fsize] += win.astype(F64) * y[row0 + m]
                            env[m * hop:m * hop + fsize] += win.astype(F64) ** 2
                        ind = buf[left:left + n] / (env[left:left + n] if norm else 1.0)
                        assert np.allclose(ref[s0:s0 + n], ind, rtol=1e-12, atol=1e-12)
                for fma in (0, 1):
                    got = A.ola_f32(y, win, segs, rows, out_len, fsize, hop, mode, norm, fma)
                    if integer:
                        assert np.array_equal(got.astype(F64), ref), "class E is not exact"
                    else:
                        ratios.append(ratio(got, ref, tol))
                if norm:
                    bad, _ = A.ola_bounds(y, win, segs, rows, out_len, fsize, hop, mode, norm, skip_norm_div=True)
                    assert ratio(got, bad, tol) > 1.0, "a missing norm division goes unnoticed"
                if fsize > hop:
                    bad, _ = A.ola_bounds(y, win, segs, rows, out_len, fsize, hop, mode, norm, m_lo_plus=0)
                    assert ratio(got, bad, tol) > 1.0, "a frame too many goes unnoticed"
    held_and_tight(ratios, 0.1, "ola_gather")


def test_ola_envelope_branch():
    rs = np.random.RandomState(9)
    segs, rows, win, y = ola_case(rs, 8, 8, [1, 2, 9], False)
    win[2] = win[5] = 0.0
    ref, tol = A.ola_bounds(y, win, segs, rows, int(segs[-1][2] + segs[-1][3]), 8, 8, 1, 1)
    assert np.isfinite(ref).all() and (ref[2::8] == 0).all() and (tol[2::8] == A.FLOOR).all()


# ------------------------------------------------------------------ resample
def resample_case(rs, integer, n_valid):
    filters, weights = A.resample_hand_filters(rs, integer)
    n_in = [A.n_in_for_valid(n_valid, int(P), int(Q)) + (i % 2) for i, (P, Q) in enumerate(filters[:, :2])]
    table, tiles = A.resample_segment_table(n_in, list(range(len(filters))), filters, A.RS_TILE)
    x = np.full(int(table[-1][0] + (table[-1][1] + 3) // 4 * 4), np.nan, F32)
    for in0, n, *_ in table:
        x[in0:in0 + n] = rs.randint(-4, 5, n) if integer else A.rfull(rs, (n,), -3, 3)
    return filters, weights, table, tiles, x


def test_resample_tables_lengths_and_refusals():
    filters = np.array([[160, 441, 9, 4, 0, 0], [1, 3, 4, 2, 0, 0]], np.int64)
    assert A.resample_segment_table([600, 2], [0, 1], filters, 256) is None        # n = 2 at 1/3: n_valid 0
    assert A.resample_segment_table([600], [2], filters, 256) is None
    t, tiles = A.resample_segment_table([600, 3, 5], [0, 1, 1], filters, 256)
    assert t[:, 3].tolist() == [218, 1, 2] and t[:, 4].tolist() == [217, 1, 1]
    assert t[:, 0].tolist() == [0, 600, 604] and t[:, 2].tolist() == [0, 220, 224]
    assert tiles.tolist() == [[0, 0], [1, 0], [2, 0]]
    bad, _ = A.resample_segment_table([600, 3, 5], [0, 1, 1], filters, 256, ceil_valid=True)
    assert not np.array_equal(bad, t), "n_valid taken as the ceiling goes unnoticed"
    assert A.resample_lds_floats(160, 441, 9) == 720       # (255 * 441 + 159) // 160 + 1 + 9 + 4 = 717, up to a multiple of 4
    assert A.resample_lds_floats(1, 64, 16) == 16344 and A.resample_lds_floats(1, 65, 16) is None and A.resample_lds_floats(0, 1, 1) is None


@pytest.mark.parametrize("n_valid", A.CASES["resample_n_valid"])
def test_resample_bound_class_e_and_a_dropped_tap(n_valid):
    rs = np.random.RandomState(10 + n_valid)
    filters, weights, table, tiles, x = resample_case(rs, True, n_valid)
    ref, tol, written = A.resample_bounds(np.nan_to_num(x), table, filters, weights)
    for fma in (0, 1):
        assert np.array_equal(A.resample_f32(np.nan_to_num(x), table, filters, weights, fma).astype(F64), ref)
    for in0, n, out0, n_out, nv, f in table:                             # independent: zero-stuffed convolution, per output
        P, Q, taps, base, woff, _ = filters[f]
        xp = np.concatenate([np.zeros(taps), np.nan_to_num(x[in0:in0 + n]).astype(F64), np.zeros(taps + 2)])
        for t in (0, nv // 2, nv - 1):
            m, ph = divmod(t * Q, P)
            w = weights[woff + ph * taps:woff + (ph + 1) * taps].astype(F64)
            assert ref[out0 + t] == np.dot(w, xp[taps + m - base:taps + m - base + taps])
        assert not ref[out0 + nv:out0 + n_out].any()
    bad, _, _ = A.resample_bounds(np.nan_to_num(x), table, filters, weights, drop_tap=0)
    assert not np.array_equal(bad, ref), "a dropped tap goes unnoticed"
    bt, _ = A.resample_segment_table(table[:, 1].tolist(), table[:, 5].tolist(), filters, A.RS_TILE, ceil_valid=True)
    assert (bt[:, 4] > table[:, 4]).any()
    filters, weights, table, tiles, x = resample_case(rs, False, n_valid)
    ref, tol, _ = A.resample_bounds(np.nan_to_num(x), table, filters, weights)
    ratios = [ratio(A.resample_f32(np.nan_to_num(x), table, filters, weights, fma), ref, tol) for fma in (0, 1)]
    assert max(ratios) <= 1.0 and max(ratios) >= 0.02
    lds = max(A.resample_lds_floats(int(P), int(Q), int(tp)) for P, Q, tp in filters[:, :3])
    geo = A.resample_geometry(table, filters, lds)
    assert geo["g0_negative"] >= 1 and geo["edge_loads"] >= 1 and geo["unaligned"] >= 1 and geo["tail"] >= 1
    if n_valid > 256:
        assert geo["tiles"] > len(table) and geo["partial"] >= 1


# ------------------------------------------------------------------ volume
def test_volume_order_is_bit_determined_and_within_the_summation_bound():
    rs = np.random.RandomState(11)
    n_outs = [1, 7, 2047, 2048, 2049, 4100, 5]
    segs, tiles, first = A.volume_table(n_outs)
    assert first.tolist() == [0, 1, 2, 3, 4, 6, 9, 10]
    y = np.zeros(int(segs[-1][2] + 8), F32)
    for s, (_, n, out0, *_r) in enumerate(segs):
        y[out0:out0 + n] = 0.0 if s == 1 else A.rfull(rs, (n,), -12, -4) * (1000.0 if s == 2 else 1.0)
    for inc in (0, 1):
        b = A.volume_bounds(y, segs, tiles, first, -30.0, inc)
        assert ratio(b["part"], b["part_sum"], b["tol_part"] + A.FLOOR) <= 1.0
        assert ratio(b["ms"], b["ms_true"], b["tol_ms"] + A.FLOOR) <= 1.0
        assert b["silent"].tolist() == [0, 1, 0, 0, 0, 0, 0] and b["gain"][1] == 1.0
        assert (b["gain"][2] == 1.0) == bool(inc) and b["gain"][2] <= 1.0           # the loud segment
        for s in (0, 3, 5):
            ms = np.mean(y[segs[s][2]:segs[s][2] + segs[s][3]].astype(F64) ** 2)
            assert abs(b["gain"][s] - 10 ** ((-30.0 - 10 * np.log10(ms)) / 20)) <= 1e-12 * b["gain"][s]
            assert b["tol_gain"][s] < 1.01 * A.EPS32 * b["gain"][s]


# ------------------------------------------------------------------ log_power
def log_power_case(rs, rows, nb, nbp, floor):
    x = A.rfull(rs, (rows, 2 * nbp), -6, 4)
    x[:, nb:nbp] = np.nan
    x[:, nbp + nb:] = np.nan                                             # the padding bins are loaded and never used
    k = max(1, rows * nb // 4)
    idx = rs.permutation(rows * nb)[:k]
    r, j = idx // nb, idx % nb
    x[r, j] = A.rfull(rs, (k,), -14, -10)
    x[r, nbp + j] = A.rfull(rs, (k,), -14, -10)                          # powers far below the floor
    x[0, 0], x[0, nbp] = F32(np.sqrt(floor)), 0.0                        # at the floor
    return x


def test_log_power_bound_floor_and_padding():
    rs = np.random.RandomState(12)
    ratios = []
    floor = 2.0 ** -20
    for rows, nb, nbp in A.CASES["log_power"]:
        x = log_power_case(rs, rows, nb, nbp, floor)
        p, tp, l, tl, below = A.log_power_bounds(np.nan_to_num(x), nb, nbp, floor)
        assert not p[:, nb:].any() and not l[:, nb:].any() and (below.any() or rows * nb < 4)
        assert np.allclose(l[:, :nb], np.log(np.maximum(np.abs(x[:, :nb].astype(F64) + 1j * x[:, nbp:nbp + nb]) ** 2, floor)), rtol=1e-13, atol=1e-13)
        for fma in (0, 1):
            for push in (-1, 0, 1):
                gp, gl = A.log_power_f32(np.nan_to_num(x), nb, nbp, floor, fma, push)
                ratios.append(ratio(gl, l, tl))
                assert ratio(gp, p, tp) <= 1.0
                assert len(np.unique(gl[below].view(np.int32))) <= 1
    held_and_tight(ratios, 0.25, "log_power")


# ------------------------------------------------------------------ voicing
@pytest.mark.parametrize("pattern", ["all", "none", "alt", "last_of_chunk", "first_of_next", "edges"])
def test_voicing_class_e_is_exact_and_strict_comparison_shows(pattern):
    for M, nlag in ((513, 65), (257, 206), (64, 1), (1, 63)):
        r, gain, mc = A.voicing_e_case(M, nlag, pattern, 5, ldr=nlag + 3, ldm=28)
        segs = A.seg_table([M], [0])
        b = A.voicing_bounds(np.nan_to_num(r), nlag, np.nan_to_num(gain), mc, segs, 0.5, 2.0 ** -4)
        r32 = np.nan_to_num(r)
        pk32 = (r32[:, 1:nlag + 1] * np.nan_to_num(gain)[None, 1:nlag + 1]).max(1).clip(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            p32 = np.where(r32[:, 0] > 0, pk32 / r32[:, 0], F32(0))
        assert np.array_equal(p32.astype(F64), b["peak"]), "class E: the fp32 quotient is not exact"
        v = b["voiced"].astype(bool)
        f = np.arange(M)
        want = {"all": np.ones(M, bool), "none": np.zeros(M, bool), "alt": f % 2 == 0, "last_of_chunk": f % 256 == 255,
                "first_of_next": (f % 256 == 0) & (f > 0)}.get(pattern)
        if want is not None:
            assert np.array_equal(v, want)
        assert b["count"][0] == v.sum()
        assert np.array_equal(b["feats"][:v.sum()], mc[v, :24]) and np.isnan(b["feats"][v.sum():]).all()
        if M > 8 and pattern in ("all", "alt", "edges"):
            s = A.voicing_bounds(np.nan_to_num(r), nlag, np.nan_to_num(gain), mc, segs, 0.5, 2.0 ** -4, strict=True)
            assert s["count"][0] < b["count"][0], "> for >= goes unnoticed: no frame sits on peak == peak_min"
    assert A.voicing_geometry(513) == dict(chunks=3, partial_chunk=True, partial_wave=True)


def voicing_r_case(rs, M, nlag):
    r = np.abs(A.rfull(rs, (M, nlag + 1), -3, 1))
    r[:, 0] = np.abs(A.rfull(rs, (M,), -4, 6))
    r[:, 1:] *= r[:, :1] * rs.uniform(0.05, 0.6, (M, 1)).astype(F32)
    r[:, 1:] *= rs.choice([-1.0, 1.0], (M, nlag)).astype(F32)
    r[rs.randint(0, M), 0] = 0.0
    gain = (1.0 + rs.rand(nlag + 1)).astype(F32)
    mc = A.rfull(rs, (M, 24))
    return r, gain, mc


def test_voicing_class_r_leaves_at_most_one_percent_undecided():
    rs = np.random.RandomState(13)
    for M in A.CASES["voicing_M"]:
        for nlag in (1, 65, 206):
            r, gain, mc = voicing_r_case(rs, M, nlag)
            b = A.voicing_bounds(r, nlag, gain, mc, A.seg_table([M], [0]), 0.45, 0.01)
            assert (~b["decided"]).sum() <= 0.01 * M
            if M > 60:
                assert 0 < b["count"][0] < M


# ------------------------------------------------------------------ DTW
def dtw_r_case(nx, ny):
    rs = np.random.RandomState(1000 * nx + ny)
    return A.rfull(rs, (nx, 24), -2, 2), A.rfull(rs, (ny, 24), -2, 2), A.rfull(rs, (nx,), 0, 3), A.rfull(rs, (ny,), 0, 3)


@pytest.mark.parametrize("nx,ny", A.CASES["dtw_r"])
def test_dtw_reference_margins_hold_on_every_r_case(nx, ny):
    x, y, lx, ly = dtw_r_case(nx, ny)
    d = A.dtw_full(x, y, lx, ly)
    assert d["margin_ok"], f"smallest decision margin {d['min_margin']} is within the bound: the case would be dropped"
    assert d["bound"] <= (28 + 2 * (nx + ny)) * 2.0 ** -53 * d["cost"] * 1.001 + A.FLOOR or nx * ny < 9
    if nx * ny <= 300 * 300:
        from test_mcd import dtw_ref
        from test_f0 import dtw_payload_ref
        c, l = dtw_ref(x, y)
        assert abs(c - d["cost"]) <= d["bound"] and l == d["length"]
        _, _, sse = dtw_payload_ref(x, y, lx, ly)
        assert abs(sse - d["sse"]) <= 1e-12 * sse
    f = A.dtw_full(x, y, dist_dtype=F32)
    if nx * ny > 4:
        assert abs(f["cost"] - d["cost"]) > d["bound"], "an fp32 dist_row goes unnoticed"
    g_ = A.dtw_geometry(nx, ny)
    assert g_["swap"] == (nx > ny) and g_["slots"] == -(-min(nx, ny) // 256)


def test_dtw_small_against_brute_force():
    from test_mcd import dtw_brute
    for nx, ny in ((1, 1), (1, 5), (5, 1), (2, 2), (4, 6)):
        x, y, _, _ = dtw_r_case(nx, ny)
        c, l = dtw_brute(x, y)
        d = A.dtw_full(x, y)
        assert abs(c - d["cost"]) <= d["bound"] and l == d["length"]
    assert np.isnan(A.dtw_full(np.zeros((0, 24)), np.zeros((3, 24)))["cost"])


def test_dtw_tie_cases_tie_where_they_say_and_a_flipped_preference_shows():
    for name, (x, y, want) in A.dtw_e_cases().items():
        d = A.dtw_full(x, y)
        assert d["cost"] == int(d["cost"]) and d["bound"] < 1e-9
        kind = name.rsplit("_", 1)[0]
        if kind == "equal":
            assert d["length"] == want and d["ties"]["all3"] >= min(len(x), len(y)) - 1
            assert A.dtw_full(x, y, order=(2, 0, 1))["length"] == max(len(x), len(y)), "a diagonal-first tie goes unnoticed"
        elif kind == "mixed":
            for k, o in A.DTW_TIE_ORDERS.items():
                assert d["ties"][k] >= 1 and A.dtw_full(x, y, order=o)["length"] != d["length"], (name, k)
            assert A.dtw_geometry(len(x), len(y))["slots"] == 2
        else:
            assert d["ties"][kind] >= 1 and sum(d["ties"].values()) == d["ties"][kind], f"{name}: {d['ties']}"
            assert A.dtw_full(x, y, order=A.DTW_TIE_ORDERS[kind])["length"] != d["length"]
        assert A.dtw_full(y, x)["cost"] == d["cost"]                     # run both ways round on the GPU: both swap paths


# ------------------------------------------------------------------ Viterbi
def test_viterbi_case_reaches_what_it_names_and_a_last_on_tie_shows():
    r, gain, v, segs = A.viterbi_e_case()
    l2, oc = A.viterbi_tables()
    rz, gz = np.nan_to_num(r), np.nan_to_num(gain)
    b = A.viterbi_ref(rz, gz, v, segs, l2, oc, 0.5, 16000.0, 20)
    lens = [e - a + 1 for a, e in b["runs"]]
    assert lens[:5] == list(A.VIT_RUNS) and b["runs"][4][1] == segs[0][1] - 1          # the last run ends on the last frame
    assert [-(-n // A.F0_CHUNK) for n in A.VIT_RUNS] == [1, 1, 1, 2, 3]                # traceback chunks
    M0 = int(segs[0][1])
    assert set(np.unique(b["lag"][:M0])) == {0, 20 + A.VIT_PAIRS[0], 20 + A.VIT_PAIRS[1]}, "a tie went to the second state"
    assert (np.diff(b["lag"][:M0][v[:M0] != 0]) != 0).sum() > 100                      # the path jumps
    want = {"first_state": 0.0, "last_state": 0.0, "not_concave": 0.0, "clamp_low": -0.5, "clamp_high": 0.5, "inside": 0.1}
    for i, (name, m) in enumerate(A.VIT_WINNERS.items()):
        rows = slice(M0 + 4 * i + 1, M0 + 4 * i + 4)
        assert (b["lag"][rows] == 20 + m).all() and np.allclose(b["f0"][rows], 16000.0 / (20 + m + want[name]), rtol=1e-15), name
    assert np.isnan(b["lf0v"][segs[2][0]:]).all() and (b["lag"][segs[2][0]:] == 0).all()
    nv = [(v[a:a + n] != 0).sum() for a, n in segs[:, :2]]
    for (row0, M, _, _), n in zip(segs, nv):                             # lf0v: ln f0 of the voiced frames, packed at row0
        lf = b["lf0v"][row0:row0 + M]
        assert np.isfinite(lf[:n]).all() and np.isnan(lf[n:]).all()
        assert np.allclose(lf[:n], np.log(b["f0"][row0:row0 + M][v[row0:row0 + M] != 0]), atol=1e-7)
    for x in (rz[v != 0][:, :207] * 8, gz[1:207], l2 * 8, oc):                            # class E: dyadic inputs
        assert np.array_equal(x, np.round(x))
    bad = A.viterbi_ref(rz, gz, v, segs, l2, oc, 0.5, 16000.0, 20, last_on_tie=True)
    assert (bad["lag"] != b["lag"]).sum() > 500, ">= for > in the recurrence goes unnoticed"
    z = A.viterbi_ref(rz, gz, v, segs, l2, oc, 0.0, 16000.0, 20)         # jump_cost = 0: the frame-wise arg-max
    s = rz[:M0, 1:207] * gz[None, 1:207] / rz[:M0, :1] - oc[None, :]
    assert np.array_equal(z["lag"][:M0][v[:M0] != 0], 20 + np.argmax(s, 1)[v[:M0] != 0])


def test_viterbi_restatement_against_brute_force_and_the_existing_one():
    import itertools
    from test_f0 import viterbi_run
    rs = np.random.RandomState(3)
    l2, oc = A.viterbi_tables()
    live = (3, 9, 30)
    oc = np.full(A.F0_STATES, 1e6)
    oc[list(live)] = 0.0
    r = np.zeros((4, 207), F32)
    r[:, 0] = 1.0
    r[:, 1:] = rs.randint(0, 5, (4, 206))
    gain = np.ones(207, F32)
    b = A.viterbi_ref(r, gain, np.ones(4, np.int32), A.seg_table([4], [0]), l2, oc, 0.5, 16000.0, 20)
    s = r[:, 1:].astype(F64) - oc[None, :]
    best = max(itertools.product(live, repeat=4),
               key=lambda p: sum(s[k, p[k]] for k in range(4)) - 0.5 * sum(abs(l2[p[k]] - l2[p[k - 1]]) for k in range(1, 4)))
    obj = lambda p: sum(s[k, p[k]] for k in range(4)) - 0.5 * sum(abs(l2[p[k]] - l2[p[k - 1]]) for k in range(1, 4))  # noqa: E731
    assert obj(tuple(b["lag"] - 20)) == obj(best)
    st, _ = viterbi_run(s, l2, 0.5)
    assert np.array_equal(st, b["lag"] - 20)


# ------------------------------------------------------------------ which path
def test_named_shapes_reach_the_paths_they_name():
    geo = [A.transpose_geometry(M, C) for M, C in A.CASES["transpose"]]
    assert any(g_["tiles"] == (1, 1) and g_["partial"] == (False, False) for g_ in geo)          # 32 x 32: one full tile
    assert any(g_["partial"] == (True, True) and g_["tiles"] == (1, 2) for g_ in geo)            # 31 x 33
    assert any(g_["partial"] == (True, True) and g_["tiles"] == (2, 1) for g_ in geo)            # 33 x 31
    assert any(g_["tiles"] == (3, 3) for g_ in geo)                                              # 65 x 80
    flat = [A.flat_geometry(r * n) for r, n in A.CASES["rows_nbp"]]
    assert flat[0]["blocks"] == 1 and any(f["blocks"] > 1 and f["idle_tail"] for f in flat)      # rows nbp crosses 256
    lp = [A.flat_geometry(r * (nbp // 4)) for r, nb, nbp in A.CASES["log_power"]]
    assert any(f["blocks"] > 1 for f in lp)
    for fsize, hop, left, ns in A.CASES["frames_seg"]:                   # one 256-thread block spans all three utterances
        Ms = [A.frames_count(n, fsize, hop, left) for n in ns]
        first_block_rows = 256 // (fsize // 4)
        assert first_block_rows > Ms[0] + Ms[1], (fsize, hop)
    vg = [A.voicing_geometry(M) for M in A.CASES["voicing_M"]]
    assert {v["chunks"] for v in vg} == {1, 2, 3} and any(not v["partial_wave"] for v in vg)
    dg = [A.dtw_geometry(nx, ny) for nx, ny in A.CASES["dtw_r"]]
    assert {d["slots"] for d in dg} == {1, 2, 3} and {d["swap"] for d in dg} == {True, False}
    for taps, P, Q in A.CASES["resample_filters"]:
        assert A.resample_lds_floats(P, Q, taps) is not None
