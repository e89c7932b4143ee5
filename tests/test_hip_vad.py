"""Silence trimming on the MI355X (csrc/vad.hip: dvae_vad_trim) through the C ABI and the Python entry points of
dvae_amd.preprocess, against the float64 / integer restatement of tests/vad_ref.py.

The window energies are held to |E_dev - E_ref| <= 4 * 480 * 2^-53 * E_ref: every term of the sum is non-negative, so a
480-term float64 sum in any order is within n u of the exact one; the factor 4 covers the two orders (the device's lanes and
tree, numpy's pairwise sum) and the contraction of the multiply-subtract and the multiply-add.  Everything behind the
energies is integer logic and is compared exactly, over every window, after an assertion on the reference alone that no
energy lies within 1e-9 (relative) of a power of two, where the two sums could fall into different bins.  The compacted
signal is compared bit for bit; every buffer a launch may write is a guarded one of tests/kernel_harness.py."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_ref as V  # noqa: E402
from kernel_harness import assert_same_bits, Buf, EINVAL, F32, guards, ibuf, L, ok, ROOT, st, untouched, Worst  # noqa: E402

WORST = Worst("the silence-trimming kernels")
E_TOL = 4 * 480 * 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    WORST.report()


def held_energies(got, ref, what):
    """|E_dev - E_ref| <= 4 * 480 * 2^-53 * E_ref; a window of zeros has the energy 0 exactly"""
    zero = ref == 0
    assert (got[zero] == 0).all(), what
    WORST.note("E", got, ref, E_TOL * ref, what, skip=zero)


# ------------------------------------------------------------------------------------------------------------ the cases
def _cases():
    """name -> fp32 utterance; built once, the references with them (CASES, REFS below)"""
    rs = np.random.RandomState(20)
    c = {}
    for n in (1, 479, 480, 481, 959, 960):
        c[f"n={n}"] = V.burst(rs, n).astype(F32)
    for W in (4, 5, 7, 8, 9):
        c[f"loud W={W}"] = V.burst(rs, W * 480).astype(F32)
    y = V.burst(rs, 20 * 480).astype(F32)
    y[7 * 480 - 1:8 * 480] = 0.0                                       # with its predecessor: E_7 is exactly 0
    c["zero window inside speech"] = y
    c["all floor"] = V.floor_noise(rs, 40 * 480 + 11).astype(F32)
    c["deep silence"] = V.floor_noise(rs, 12 * 480, dbfs=-95.0).astype(F32)
    c["all zero"] = np.zeros(9 * 480 + 5, F32)
    # flag runs 5 / 6 windows apart are masked runs 6 / 7 apart: bridged / one window left out
    c["gap 6"] = V.utterance(rs, 60, [(8, 20), (25, 40)])
    c["gap 7"] = V.utterance(rs, 60, [(8, 20), (26, 40)])
    c["long edges"] = V.utterance(rs, 50, [(12, 30)])                  # 12 and 20 windows of floor around the speech
    c["tail 479"] = V.utterance(rs, 33, [(5, 14), (20, 29)], tail=479)
    c["W=20001"] = V.utterance(rs, 20001, [(3, 250), (256, 270), (500, 5000), (5007, 9000), (15000, 19999)])
    return c


CASES = _cases()
REFS = {k: V.detect(v) for k, v in CASES.items()}
SMALL = [k for k in CASES if k != "W=20001"]


def test_the_references_stay_clear_of_the_bin_borders_and_cover_the_paths():
    for k, r in REFS.items():
        if r["W"]:
            assert V.pow2_distance(r["E"]).min() > 1e-9, k               # zero exclusions: no window is left out below
    K = {k: r["K"] for k, r in REFS.items()}
    assert [REFS[f"n={n}"]["W"] for n in (1, 479, 480, 481, 959, 960)] == [0, 0, 1, 1, 1, 2]
    assert [K[f"loud W={W}"] for W in (4, 5, 7, 8, 9)] == [0, 5, 7, 8, 9]
    assert K["zero window inside speech"] == 20 and REFS["zero window inside speech"]["b"][7] == 0
    assert K["all floor"] == 40 and REFS["all floor"]["t"] == 66 and K["deep silence"] == 0 and K["all zero"] == 0
    for name, loud in (("gap 6", [(8, 20), (25, 40)]), ("gap 7", [(8, 20), (26, 40)]), ("long edges", [(12, 30)])):
        assert np.array_equal(REFS[name]["keep"], V.expected_keep(len(REFS[name]["keep"]), loud)), name
    assert REFS["gap 6"]["keep"][5:42].all() and K["gap 6"] == 37
    assert np.nonzero(REFS["gap 7"]["keep"][5:42] == 0)[0].tolist() == [17] and K["gap 7"] == 36
    assert np.nonzero(REFS["long edges"]["keep"])[0].tolist() == list(range(9, 32))
    assert REFS["tail 479"]["W"] == 33 and REFS["W=20001"]["W"] == 20001 and 0 < K["W=20001"] < 20001


# --------------------------------------------------------------------------------------------------------- C ABI harness
def _tables(ns):
    """segment table {., ., out0, n_out, ., .} packed at multiples of 4, the window map and each segment's first window"""
    table = np.zeros((len(ns), 6), np.int64)
    off = 0
    for s, n in enumerate(ns):
        table[s, 2], table[s, 3] = off, n
        off += (n + 3) // 4 * 4
    W = table[:, 3] // 480
    first = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    wins = np.array([(s, w) for s in range(len(ns)) for w in range(W[s])], np.int64).reshape(-1, 2)
    return table, wins, first, max(4, off)


class Run:
    """one dvae_vad_trim launch on the utterances `names`: NaN in the gaps of the input, every output guarded"""

    def __init__(self, names, optional=True):
        self.names = names
        ys = [CASES[k] for k in names]
        self.table, wins, self.first, total = _tables([len(y) for y in ys])
        self.nseg, self.nwin = len(ys), int(self.first[-1])
        host = np.full(total, np.nan, F32)
        for y, o in zip(ys, self.table[:, 2]):
            host[o:o + len(y)] = y
        self.y, self.out = Buf(data=host), Buf((total,))
        self.segs, self.wins, self.wfirst = ibuf(self.table), ibuf(wins if len(wins) else np.zeros((1, 2))), ibuf(self.first)
        nw = max(1, self.nwin)
        self.E = Buf((nw,), torch.float64) if optional else None
        self.flags = Buf((nw,), torch.int32) if optional else None
        self.t = Buf((self.nseg,), torch.int32) if optional else None
        self.bins, self.keep, self.dst = (Buf((nw,), torch.int32) for _ in range(3))
        self.K = Buf((self.nseg,), torch.int32)
        self.written = (self.out, self.E, self.bins, self.flags, self.keep, self.dst, self.t, self.K)

    def args(self, **k):
        g = lambda name, dflt: k.get(name, dflt)
        p = lambda b: None if b is None else b.ptr
        return [g("y", self.y.ptr), g("out", self.out.ptr), g("segs_host", self.table.ctypes.data), self.segs.ptr,
                g("nseg", self.nseg), self.wins.ptr, g("nwin", self.nwin), self.wfirst.ptr, g("E", p(self.E)),
                g("bins", self.bins.ptr), p(self.flags), g("keep", self.keep.ptr), self.dst.ptr, p(self.t),
                g("K", self.K.ptr), st()]

    def launch(self):
        ok(L().dvae_vad_trim(*self.args()), "dvae_vad_trim")
        guards(self.y, *self.written)
        return self

    def check(self, what):
        """everything against REFS, exactly but for the energies; nothing written that the contract does not name"""
        got_out, out_bits = self.out.np(), self.out.bits()
        bins, keep, dst, K = self.bins.np(), self.keep.np(), self.dst.np(), self.K.np()
        claimed = np.zeros(out_bits.shape, bool)
        for s, name in enumerate(self.names):
            r, a, b = REFS[name], int(self.first[s]), int(self.first[s + 1])
            assert b - a == r["W"]
            if self.E is not None:
                held_energies(self.E.np()[a:b], r["E"], f"{what}: {name}")
                assert np.array_equal(self.flags.np()[a:b], r["flags"]), (what, name, "flags")
                assert self.t.np()[s] == r["t"], (what, name, "t", self.t.np()[s], r["t"])
            assert np.array_equal(bins[a:b], r["b"]), (what, name, "bins")
            assert np.array_equal(keep[a:b], r["keep"]), (what, name, "keep")
            assert np.array_equal(dst[a:b], r["dst"]), (what, name, "dst")
            assert K[s] == r["K"], (what, name, "K", K[s], r["K"])
            o = int(self.table[s, 2])
            assert_same_bits(got_out[o:o + 480 * r["K"]], V.trim(CASES[name], r), f"{what}: {name}: the kept windows")
            claimed[o:o + 480 * r["K"]] = True                          # 480 K is a multiple of 4: no pad floats behind it
        untouched(out_bits[~claimed], f"{what}: out beyond the kept windows")
        if self.nwin == 0:
            for b in (self.E, self.bins, self.flags, self.keep, self.dst):
                assert b is None or b.poisoned().all()


def _bits_of(run):
    """every output of a run, per segment, as bytes"""
    per = []
    for s in range(run.nseg):
        a, b, o = int(run.first[s]), int(run.first[s + 1]), int(run.table[s, 2])
        K = int(run.K.np()[s])
        per.append((run.E.bits()[a:b].tobytes(), run.bins.np()[a:b].tobytes(), run.flags.np()[a:b].tobytes(),
                    run.keep.np()[a:b].tobytes(), run.dst.np()[a:b].tobytes(), int(run.t.np()[s]), K,
                    run.out.bits()[o:o + 480 * K].tobytes()))
    return per


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", SMALL)
def test_one_utterance_alone(name):
    Run([name]).launch().check("alone")


def test_chunk_loop_on_20001_windows():
    Run(["W=20001"]).launch().check("alone")


def test_a_batch_mixing_every_case_in_one_launch():
    Run(list(CASES)).launch().check("mixed batch")
    Run(SMALL, optional=False).launch().check("mixed batch without the optional outputs")


def test_independence_of_the_batch_and_determinism():
    names = ["gap 7", "n=479", "tail 479", "loud W=5", "all floor", "zero window inside speech", "long edges", "n=960"]
    batch = _bits_of(Run(names).launch())
    again = _bits_of(Run(names).launch())
    other = _bits_of(Run(names[::-1]).launch())[::-1]                   # other neighbours, other offsets
    assert batch == again and batch == other
    for i, name in enumerate(names):
        assert _bits_of(Run([name]).launch())[0] == batch[i], name


def test_bad_arguments_return_einval_and_write_nothing():
    r = Run(["gap 6", "n=481"])
    off4 = r.table.copy()
    off4[1, 2] += 2
    neg = r.table.copy()
    neg[0, 3] = -1
    for bad in (dict(nseg=-1), dict(y=r.y.ptr + 4), dict(out=r.out.ptr + 8), dict(out=r.y.ptr), dict(segs_host=off4.ctypes.data),
                dict(segs_host=neg.ctypes.data), dict(nwin=r.nwin + 1), dict(nwin=-1), dict(E=r.E.ptr + 4),
                dict(bins=r.bins.ptr + 2), dict(keep=None), dict(K=None), dict(y=None), dict(segs_host=None)):
        assert L().dvae_vad_trim(*r.args(**bad)) == EINVAL, bad
    guards(r.y, *r.written)
    for b in r.written:
        assert b.poisoned().all()
    assert L().dvae_vad_trim(*r.args(nseg=0, nwin=0)) == 0                # an empty batch: nothing to do
    guards(r.y, *r.written)
    for b in r.written:
        assert b.poisoned().all()
    r.launch().check("after the refusals")


# ------------------------------------------------------------------------------------------------- Python entry points
def test_vad_packed_and_trim_long_silences_batch():
    from dvae_amd.preprocess import pack, trim_long_silences_batch, vad_packed
    names = ["gap 6", "n=1", "all floor", "deep silence", "tail 479"]
    ys = [CASES[k] for k in names]
    outs, K = trim_long_silences_batch(ys)
    assert K.tolist() == [REFS[k]["K"] for k in names]
    for k, o in zip(names, outs):
        assert_same_bits(o.cpu().numpy(), V.trim(CASES[k], REFS[k]), k)
    y, offs = pack(ys)
    table = np.zeros((len(ys), 6), np.int64)
    table[:, 2], table[:, 3] = offs, [len(v) for v in ys]
    before = y.clone()
    out, K2, ex = vad_packed(y, table, want=("E", "flags", "keep", "t"))
    assert torch.equal(y, before) and K2.tolist() == K.tolist() and ex["t"].tolist() == [REFS[k]["t"] for k in names]
    first = ex["first"]
    for s, k in enumerate(names):
        a, b = int(first[s]), int(first[s + 1])
        assert np.array_equal(ex["keep"][a:b].cpu().numpy(), REFS[k]["keep"])
        assert np.array_equal(ex["flags"][a:b].cpu().numpy(), REFS[k]["flags"])
        held_energies(ex["E"][a:b].cpu().numpy(), REFS[k]["E"], f"vad_packed: {k}")
    with pytest.raises(ValueError):
        vad_packed(y, table, want=("mask",))
    assert trim_long_silences_batch([])[0] == []


# ------------------------------------------------------------------------------------------------------------ end to end
def _write_pcm16(path, x, sr):
    path.parent.mkdir(parents=True, exist_ok=True)
    v = np.clip(np.round(np.asarray(x) * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(v.tobytes())


def _speech(rs, sr, lead, talk1, pause, talk2, trail, f):
    """floor, speech, floor, speech, floor (seconds each) at rate sr: a -62 dBFS floor under tone-plus-noise speech"""
    parts = []
    for i, d in enumerate((lead, talk1, pause, talk2, trail)):
        n = int(sr * d)
        x = V.floor_noise(rs, n)
        if i % 2:
            x = x + 0.1 * np.sin(2 * np.pi * f * np.arange(n) / sr) * (1 + 0.3 * np.sin(np.arange(n) * 9.0 / sr)) + 0.01 * rs.randn(n)
        parts.append(x)
    return np.concatenate(parts)


def _tree(root):
    rs = np.random.RandomState(31)
    w = root / "VCTK-Corpus" / "wav16"
    for s, (spk, sr) in enumerate((("p301", 48000), ("p302", 16000))):
        for u in range(3):
            x = _speech(rs, sr, 0.5 + 0.2 * u, 0.5 + 0.1 * s, 0.35 + 0.25 * u, 0.4, 0.6 + 0.2 * s, 200.0 + 70 * u + 30 * s)
            _write_pcm16(w / spk / f"{spk}_{u:03d}.wav", x, sr)
    _write_pcm16(w / "p301" / "p301_floor.wav", V.floor_noise(rs, 48000), 48000)       # floor only: all of it is kept
    _write_pcm16(w / "p302" / "p302_short.wav", 0.1 * np.ones(300), 16000)             # under 30 ms
    return w


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "dvae_amd.preprocess"] + args, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def _npys(d):
    return {str(p.relative_to(d)): p.read_bytes() for p in sorted(d.rglob("*.npy"))}


def test_cli_trim_end_to_end(tmp_path):
    from dvae_amd.frontend import MelFrontend
    from dvae_amd.preprocess import _run_batch, read_wav, Resampler
    from oracle.mel_ref import melspectrogram
    from test_preprocess import normalize_ref, resample_ref
    root = tmp_path / "data"
    wav16 = _tree(root)
    o1, o600, plain = tmp_path / "b1", tmp_path / "b600", tmp_path / "plain"
    r1 = _run([str(root), "-o", str(o1), "--trim", "--batch-seconds", "1", "--workers", "1"])
    r600 = _run([str(root), "-o", str(o600), "--trim", "--batch-seconds", "600", "--workers", "16"])
    s1, s600 = _npys(o1), _npys(o600)
    assert sorted(s1) == sorted(s600) and len(s1) == 7 and all(s1[k] == s600[k] for k in s1)
    fe = MelFrontend()
    total = kept = 0
    for spk in ("p301", "p302"):
        lines = (o1 / spk / "_sources.txt").read_text().splitlines()
        assert len(lines) == (4 if spk == "p301" else 3)
        for l in lines:
            name, src = l.split(",", 1)
            x, sr = read_wav(src)
            w64, _ = normalize_ref(resample_ref(x, sr))
            ref = V.detect(w64)
            assert V.pow2_distance(ref["E"]).min() > 1e-5, name           # fp32 samples on the device, float64 here
            mel = np.load(o1 / spk / name)
            assert mel.dtype == np.float32 and mel.shape == (80, fe.num_frames(480 * ref["K"])), (name, mel.shape, ref["K"])
            want = melspectrogram(V.trim(w64, ref))
            assert mel.shape == want.shape and np.max(np.abs(mel - want)) <= 3e-4, (name, np.max(np.abs(mel - want)))
            if "floor" in name:
                assert ref["K"] == ref["W"] == 33                         # 16000 samples at 16 kHz: everything kept
            else:
                assert 5 <= ref["K"] < ref["W"] - 20                      # more than 0.6 s of its silences went
            total += len(w64)
            kept += 480 * ref["K"]
    summary = r1.stdout.strip().splitlines()[-1]
    assert summary == r600.stdout.strip().splitlines()[-1]
    assert summary.startswith("preprocess: 7 written, 0 already present, 1 skipped; "
                              f"trimmed {(total - kept) / 16000:.1f} s of {total / 16000:.1f} s; "), summary
    assert summary.endswith(f"p302_short.wav ({V.TOO_SHORT})"), summary
    # --no_trim on the same tree: the bytes of the untrimmed path, batch by batch as before
    rp = _run([str(root), "-o", str(plain), "--no_trim"])
    assert "trimmed" not in rp.stdout
    sp = _npys(plain)
    assert len(sp) == 8 and set(s1) < set(sp)
    fe2, rs = MelFrontend(), Resampler()
    for spk in ("p301", "p302"):
        files = sorted((wav16 / spk).glob("*.wav"))
        decoded = [read_wav(f) for f in files]
        res = _run_batch(fe2, rs, [d[0] for d in decoded], [d[1] for d in decoded], trim=False)
        for f, (mel, why) in zip(files, res):
            assert why is None
            got = np.load(plain / spk / f.name.replace(".wav", "_mel.npy"))
            assert got.shape == mel.shape and got.tobytes() == mel.tobytes(), f.name
