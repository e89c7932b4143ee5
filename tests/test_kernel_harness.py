"""The harness the kernel suites are judged by (tests/kernel_harness.py, tests/ref_common.py), on the CPU: a guard that misses
a stray byte, a comparison that takes -0.0 for +0.0 or a ratio that lets a NaN through would pass every kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_harness as H  # noqa: E402
import ref_common as RC  # noqa: E402

F32, F64 = np.float32, np.float64
CPU = dict(device="cpu")


# ------------------------------------------------------------------ Buf: guards
def payload_start(b):
    return b.ptr - b.raw.data_ptr()


@pytest.mark.parametrize("shape,dtype,lead", [((3, 5), torch.float32, 0), ((7,), torch.bfloat16, 0), ((2, 3), torch.float64, 64),
                                              ((1,), torch.uint8, 32)])
def test_a_byte_outside_the_payload_is_reported_and_one_inside_is_not(shape, dtype, lead):
    def fresh():
        return H.Buf(shape, dtype, lead=lead, **CPU)

    b = fresh()
    assert b.intact() and payload_start(b) >= H.PADB and b.raw.numel() - payload_start(b) - b.nbytes >= H.PADB
    H.guards(b, None)
    for where in (payload_start(b) - 1, payload_start(b) + b.nbytes, b.raw.numel() - 1, 0):
        b = fresh()
        b.raw[where] = 0
        assert not b.intact(), where
        with pytest.raises(AssertionError, match="outside its buffer"):
            H.guards(fresh(), b)
    for where in (payload_start(b), payload_start(b) + b.nbytes - 1):
        b = fresh()
        b.raw[where] = 0
        assert b.intact(), where
        H.guards(b)


def test_a_workspace_reports_a_write_into_its_slack():
    ws = H.Buf((100,), torch.uint8, **CPU)
    ws.slack_from = 64
    ws.t[:64] = 7
    assert ws.intact()
    ws.t[63] = 0xFF
    assert ws.intact()
    ws.t[64] = 7
    assert not ws.intact()
    with pytest.raises(AssertionError, match="outside its buffer"):
        H.guards(ws)
    ws.t[64] = 0xFF
    ws.t[99] = 0
    assert not ws.intact()


# ------------------------------------------------------------------ Buf: the fill
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_an_unwritten_payload_reads_back_as_nan(dtype):
    b = H.Buf((4, 3), dtype, **CPU)
    assert b.np().shape == (4, 3) and np.isnan(b.np()).all() and (b.bits() == -1).all() and b.poisoned().all()
    H.untouched(b.bits(), "fresh")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.int64])
def test_poisoned_marks_exactly_the_unwritten_elements(dtype):
    b = H.Buf((3, 4), dtype, **CPU)
    written = np.zeros((3, 4), bool)
    written[0, 1] = written[2, 3] = written[1, :] = True
    b.t[torch.from_numpy(written)] = 1
    assert np.array_equal(b.poisoned(), ~written)
    with pytest.raises(AssertionError, match="must not write"):
        H.untouched(b.bits(), "partly written")
    z = H.Buf((2,), dtype, fill=0, **CPU)
    assert z.poisoned().all() and not z.bits().any()


# ------------------------------------------------------------------ Buf: data
def test_fp32_bits_survive_the_upload():
    pattern = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC00001, 0xFFC12345, 0x7F800000, 0x3F800000], np.uint32)
    data = pattern.view(F32).reshape(7, 1)                      # -0.0, two denormals, two NaN payloads, inf, 1
    b = H.Buf(data=data, **CPU)
    assert b.shape == (7, 1) and b.dtype == torch.float32 and b.intact()
    assert np.array_equal(b.bits().view(np.uint32).reshape(-1), pattern)
    H.assert_same_bits(b, data, "upload")
    assert H.same_bits(b.np(), data)
    explicit = H.Buf((7,), torch.float32, data, **CPU)          # a shape of its own: the data is viewed as it
    assert explicit.shape == (7,) and np.array_equal(explicit.bits().view(np.uint32), pattern)
    assert np.array_equal(H.Buf(data=pattern, **CPU).bits().view(np.uint32), pattern)      # uint32 words travel as int32


def test_dtype_is_inferred_from_the_data():
    for np_dt, t_dt in ((np.float64, torch.float64), (np.int32, torch.int32), (np.int64, torch.int64), (np.uint8, torch.uint8)):
        a = np.arange(6).reshape(2, 3).astype(np_dt)
        b = H.Buf(data=a, **CPU)
        assert b.dtype == t_dt and b.shape == (2, 3) and np.array_equal(b.np(), a)
    i = H.ibuf([3, -1, 2 ** 40], **CPU)
    assert i.dtype == torch.int64 and i.np().tolist() == [3, -1, 2 ** 40]
    assert H.ibuf([3, -1], np.int32, **CPU).dtype == torch.int32
    assert H.Buf((2,), **CPU).dtype == torch.float32


def test_float64_values_are_rounded_to_nearest_even_fp32():
    one = 1.0
    vals = np.array([one + 2.0 ** -24, one + 3 * 2.0 ** -24, one + 2.0 ** -24 + 2.0 ** -40, 0.1, -1e-45, 1e39], F64)
    b = H.Buf((6,), torch.float32, vals, **CPU)                 # ties to even: down, up; above the tie: up
    want = np.array([one, one + 2.0 ** -22, one + 2.0 ** -23, F32(0.1), -1.4e-45, np.inf], F32)
    assert b.dtype == torch.float32 and H.same_bits(b.np(), want), (b.np(), want)
    with np.errstate(over="ignore"):
        assert H.same_bits(b.np(), vals.astype(F32))
    n = H.Buf((1,), torch.int64, np.array([7], np.int64), **CPU)
    assert n.np().tolist() == [7]


def test_a_bf16_upload_of_representable_values_is_exact():
    vals = RC.bf16(np.random.RandomState(0).uniform(-3, 3, (5, 8)).astype(F32))
    vals[0, :3] = [-0.0, 2.0 ** -126, 3.0]
    b = H.Buf(dtype=torch.bfloat16, data=vals, **CPU)
    assert b.dtype == torch.bfloat16 and b.esize == 2 and b.nbytes == 80 and b.np().dtype == F32
    assert H.same_bits(b.np(), vals)
    assert np.array_equal(b.bits().view(np.uint16), vals.view(np.uint32) >> 16)
    rounded = H.Buf(dtype=torch.bfloat16, data=np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], F32), **CPU)
    assert rounded.np().tolist() == [1.0, 1.0 + 2.0 ** -6]     # ties to even, as RC.bf16 has it
    assert H.same_bits(rounded.np(), RC.bf16([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]))


# ------------------------------------------------------------------ Buf: addresses
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8])
def test_addresses(dtype):
    b = H.Buf((5, 3), dtype, **CPU)
    assert b.ptr % 16 == 0 and payload_start(b) % 256 == 0 and H.P(b) == b.ptr and H.P(None) is None
    assert b.ptr == b.t.data_ptr() and b.at(0) == b.ptr and b.at(7) == b.ptr + 7 * b.esize == b.t.view(-1)[7:].data_ptr()
    room = b.raw.numel() - payload_start(b) - H.PADB                        # the payload, rounded up to 16 bytes
    assert room % 16 == 0 and 0 <= room - b.nbytes < 16
    for lead in (32, 64):
        c = H.Buf((5, 3), dtype, lead=lead, **CPU)
        assert payload_start(c) % 256 == lead and c.ptr % 16 == 0 and c.intact()


def test_pad_puts_nan_around_the_data():
    data = np.arange(6, dtype=F32).reshape(2, 3)
    p = H.Pad(data, before=4, after=8, **CPU)
    flat = p.buf.np()
    assert p.ptr == p.buf.ptr + 16 and flat.shape == (18,)
    assert np.isnan(flat[:4]).all() and np.isnan(flat[10:]).all() and np.array_equal(flat[4:10], data.reshape(-1))


# ------------------------------------------------------------------ bits
def test_same_bits_tells_zeros_and_nans_apart():
    nan1, nan2 = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(F32)
    assert H.same_bits(F32([1.0, -0.0]), F32([1.0, -0.0])) and H.same_bits(F32(0.5), 0.5)
    assert not H.same_bits(F32([0.0]), F32([-0.0]))
    assert H.same_bits(F32([nan1]), F32([nan1])) and not H.same_bits(F32([nan1]), F32([nan2]))
    assert not H.same_bits(np.zeros(4, F32), np.zeros((2, 2), F32)) and not H.same_bits(np.zeros(3, F32), np.zeros(4, F32))
    H.assert_same_bits(F32([nan1, -0.0]), F32([nan1, -0.0]), "equal")
    H.assert_same_bits(np.zeros((2, 2), F32), np.zeros(4, F32), "flattened")
    for got, ref in ((F32([0.0]), F32([-0.0])), (F32([nan1]), F32([nan2]))):
        with pytest.raises(AssertionError, match="1 of 1 elements differ in their bits, first at \\[0\\]"):
            H.assert_same_bits(got, ref, "differs")
    with pytest.raises(AssertionError, match="3 elements instead of 4"):
        H.assert_same_bits(np.zeros(3, F32), np.zeros(4, F32), "size")
    b = H.Buf(data=F32([0.0, 1.0]), **CPU)
    with pytest.raises(AssertionError, match="first at \\[0\\]"):
        H.assert_same_bits(b, F32([-0.0, 1.0]), "a buffer")
    assert H.bits(F32([-0.0])).tolist() == [0x80000000]
    assert H.dev_equal(torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0]))
    assert not H.dev_equal(torch.tensor([0.0]), torch.tensor([-0.0])) and not H.dev_equal(torch.zeros(4), torch.zeros(2, 2))
    assert H.down(torch.arange(3)).tolist() == [0, 1, 2]


# ------------------------------------------------------------------ worst_ratio
def test_worst_ratio_edges():
    inf, nan = np.inf, np.nan
    assert RC.worst_ratio([], [], []) == (0.0, -1) and RC.worst_ratio(np.zeros((0, 3)), np.zeros((0, 3)), 1.0) == (0.0, -1)
    assert RC.worst_ratio([1.0, 2.5], [1.0, 2.0], [1.0, 1.0]) == (0.5, 1)
    assert RC.worst_ratio([1.0, 2.5], [1.0, 2.0], 0.25) == (2.0, 1)                      # a scalar bound is broadcast
    for got, ref, tol in (([1.0, nan], [1.0, 1.0], [1.0, 1.0]), ([1.0, 1.0], [1.0, nan], [1.0, 1.0]), ([1.0, 1.0], [1.0, 1.0], [1.0, nan]),
                          ([1.0, inf], [1.0, 1.0], [1.0, 1.0]), ([1.0, inf], [1.0, inf], [1.0, 1.0]), ([1.0, 1.0], [1.0, 1.0], [1.0, 0.0]),
                          ([1.0, 2.0], [1.0, 1.0], [1.0, 0.0]), ([1.0, 1.0], [1.0, 1.0], [1.0, -inf])):
        for unheld in (False, True):
            assert RC.worst_ratio(got, ref, tol, inf_tol_unheld=unheld) == (inf, 1), (got, ref, tol, unheld)
    # a +inf bound: infinitely wrong, unless the caller says that nothing is held there
    assert RC.worst_ratio([1.0, 5.0], [1.0, 1.0], [1.0, inf]) == (inf, 1)
    assert RC.worst_ratio([1.5, 5.0], [1.0, 1.0], [1.0, inf], inf_tol_unheld=True) == (0.5, 0)
    assert RC.worst_ratio([1.0, nan], [1.0, 1.0], [1.0, inf], inf_tol_unheld=True) == (inf, 1)      # ... but a NaN is still one
    import bn_ref                                               # ... which is what bn_ref, elem_ref and audio_ref export
    assert bn_ref.worst_ratio([1.5, 5.0], [1.0, 1.0], [1.0, inf]) == (0.5, 0)
    got, ref = np.zeros((3, 4)), np.zeros((3, 4))
    got[2, 1], got[0, 3] = 0.5, -0.25
    assert RC.worst_ratio(got, ref, np.full((3, 4), 0.5)) == (1.0, 9)                    # a flat index into [3, 4]


def test_worst_ratio_is_what_the_four_earlier_ones_returned():
    """On finite values and positive bounds: the bodies tests/lstm_ref.py, tests/bn_ref.py, tests/adam_ref.py and
    tests/ema_ref.py had, restated."""
    def lstm(got, ref, tol):
        ref = np.asarray(ref, F64)
        got, tol = np.asarray(got, F64), np.broadcast_to(np.asarray(tol, F64), ref.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(got - ref) / tol
        r = np.where(np.isfinite(got) & np.isfinite(ref) & np.isfinite(tol) & ~np.isnan(r), r, np.inf)
        i = int(np.argmax(r))
        return float(r.reshape(-1)[i]), i

    def bn(got, ref, tol):
        ref = np.asarray(ref, F64)
        got, tol = np.asarray(got, F64), np.broadcast_to(np.asarray(tol, F64), ref.shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.abs(got - ref) / tol
        r = np.where(np.isposinf(tol), 0.0, r)
        r = np.where(np.isfinite(got) & np.isfinite(ref) & ~np.isnan(tol) & ~np.isnan(r), r, np.inf)
        i = int(np.argmax(r))
        return float(r.reshape(-1)[i]), i

    def adam(got, ref, tol):
        r = np.abs(np.asarray(got, np.float64) - ref) / tol
        i = int(np.argmax(r))
        return float(r[i]), i

    def ema(got, ref, tol):
        r = np.abs(np.asarray(got, dtype=np.float64) - ref) / tol
        i = int(np.argmax(r))
        return float(r[i]), i

    rs = np.random.RandomState(5)
    n = 10000
    ref = rs.standard_normal(n) * 10.0 ** rs.randint(-6, 7, n)
    tol = np.abs(ref) * 2.0 ** -24 * rs.uniform(0.5, 8, n) + 2.0 ** -126
    got = (ref + tol * rs.uniform(-1.5, 1.5, n)).astype(F32)
    want = lstm(got, ref, tol)
    assert want[0] > 1.0 and np.isfinite(want[0])
    for old in (bn, adam, ema):
        assert old(got, ref, tol) == want
    assert RC.worst_ratio(got, ref, tol) == want and RC.worst_ratio(got, ref, tol, inf_tol_unheld=True) == want
    shape = (100, 100)
    want2 = lstm(got.reshape(shape), ref.reshape(shape), tol.reshape(shape))
    assert want2 == want == bn(got.reshape(shape), ref.reshape(shape), tol.reshape(shape))
    assert RC.worst_ratio(got.reshape(shape), ref.reshape(shape), tol.reshape(shape)) == want
    for k in range(0, n, 1000):                                 # and on every tenth of the draws, where the worst lies elsewhere
        s = slice(k, k + 1000)
        assert RC.worst_ratio(got[s], ref[s], tol[s]) == lstm(got[s], ref[s], tol[s]) == adam(got[s], ref[s], tol[s])


def test_bf16_and_split3():
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0, 3.14159274], F32)
    assert RC.bf16(x).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -0.0, 3.140625]
    assert RC.bf16_trunc(x).tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, -0.0, 3.140625]
    r = np.random.RandomState(1).standard_normal(1000).astype(F32)
    planes = RC.split3(r)
    assert all((p.view(np.uint32) & 0xFFFF == 0).all() for p in planes)
    assert np.array_equal(planes[0].astype(F64) + planes[1].astype(F64) + planes[2].astype(F64), r.astype(F64))
    assert RC.g(3) == 3 * 2.0 ** -24 / (1 - 3 * 2.0 ** -24)


# ------------------------------------------------------------------ Worst
def test_worst_note_asserts_at_one_and_records_the_maximum():
    w = H.Worst("a module")
    ref, tol = np.zeros((2, 3)), np.full((2, 3), 0.5)
    got = ref.copy()
    got[1, 1] = 0.5
    assert w.note("q", got, ref, tol, "exactly the bound") == 1.0 and w.worst == {"q": 1.0}
    w.note("q", ref, ref, tol, "exact")
    assert w.worst == {"q": 1.0}                                # the maximum over the calls
    got[1, 1] = np.nextafter(0.5, 1.0)
    with pytest.raises(AssertionError, match=r"just above: q at flat index 4: .*0\.5000000000000001.*, reference .*0\.0.*, bound 0\.5, error / bound = 1\.000"):
        w.note("q", got, ref, tol, "just above")
    assert w.worst["q"] > 1.0                                   # recorded before it fails
    got[1, 1] = np.nan
    with pytest.raises(AssertionError, match="error / bound = inf"):
        w.note("r", got, ref, 0.5, "a NaN, a scalar bound")
    w.record("s", 0.25)
    w.record("s", 0.125)
    assert w.worst["s"] == 0.25


def test_worst_note_honours_skip_and_the_ratio_rule():
    w = H.Worst("a module")
    ref, got = np.zeros((2, 3)), np.zeros((2, 3))
    got[0, 2], got[1, 0] = 9.0, 0.25
    skip = np.zeros((2, 3), bool)
    skip[0, 2] = True
    with pytest.raises(AssertionError):
        w.note("all", got, ref, 0.5, "nothing skipped")
    assert w.note("kept", got, ref, 0.5, "skipped", skip=skip) == 0.5
    assert w.note("kept by row", got, ref, 0.5, "skipped", skip=np.array([[True], [False]])) == 0.5
    assert w.note("none left", got, ref, 0.5, "skipped", skip=np.ones((2, 3), bool)) == 0.0
    tol = np.full((2, 3), 0.5)
    tol[0, 2] = np.inf
    with pytest.raises(AssertionError, match="error / bound = inf"):
        w.note("inf bound", got, ref, tol, "held by default")
    unheld = lambda g, r, t: RC.worst_ratio(g, r, t, inf_tol_unheld=True)
    assert w.note("inf bound", got, ref, tol, "not held", ratio_fn=unheld) == 0.5
    assert H.Worst("another", ratio_fn=unheld).note("inf bound", got, ref, tol, "not held") == 0.5


def test_worst_report_prints_both_formats(capsys):
    w = H.Worst("test_x.py")
    w.record("zeta", 0.5)
    w.record("alpha q", 0.12345)
    w.report()
    assert capsys.readouterr().out == "\nworst error / bound over test_x.py: zeta 0.500, alpha q 0.123\n"
    w.sort = True
    w.report()
    assert capsys.readouterr().out == "\nworst error / bound over test_x.py: alpha q 0.123, zeta 0.500\n"
    t = H.Worst("test_y.py")
    t.record(("v5 fp32", "h"), 0.25)
    t.record(("gen fp32", "c"), 0.5)
    t.record(("gen fp32", "h"), 1 / 3)
    t.report()
    assert capsys.readouterr().out == ("\nworst error / bound over test_y.py\n| kernels | h | c |\n|---|---|---|\n"
                                       "| gen fp32 | 0.333 | 0.500 |\n| v5 fp32 | 0.250 |  |\n")
