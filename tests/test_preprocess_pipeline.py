"""The CLI's host pipeline (dvae_amd.preprocess.preprocess_vctk) with the GPU passes stubbed out: decoding runs a bounded
window ahead of the batch being filled, writes start while files are still decoding, the number of decoded files held at
once does not grow with the corpus, and the outputs and `_sources.txt` lines are those of the plain order whatever the
batch size, worker count and window."""
import os
import sys
import threading
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dvae_amd  # noqa: E402,F401
from dvae_amd import preprocess  # noqa: E402


def _tree(root, n_spk=2, n_utt=20, sr=16000, seconds=1.0):
    base = root / "VCTK-Corpus" / "wav16"
    for s in range(n_spk):
        d = base / f"p{225 + s}"
        d.mkdir(parents=True)
        for u in range(n_utt):
            v = ((np.arange(int(sr * seconds)) * (s + u + 1)) % 2000 - 1000).astype("<i2")
            with wave.open(str(d / f"p{225 + s}_{u:03d}.wav"), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(sr)
                w.writeframes(v.tobytes())
    return base


class _Probe:
    """stubs for read_wav / the GPU batch / the file write, recording what ran when"""

    def __init__(self, monkeypatch, decode_s=0.005, run_s=0.0):
        self.lock = threading.Lock()
        self.events = []                 # ("decode_start" | "decode_end" | "write_start", time, path)
        self.started = self.written = 0
        self.max_held = 0                # decodes started minus files written or consumed by a batch
        self.consumed = 0
        real = preprocess.read_wav

        def read_wav(path, duration=600.0):
            with self.lock:
                self.started += 1
                self.max_held = max(self.max_held, self.started - self.consumed)
                self.events.append(("decode_start", time.perf_counter(), str(path)))
            time.sleep(decode_s)
            r = real(path, duration)
            with self.lock:
                self.events.append(("decode_end", time.perf_counter(), str(path)))
            return r

        def run_batch(wavs, srs):
            time.sleep(run_s)                # the GPU passes take time: decoders must not run away meanwhile
            with self.lock:
                self.consumed += len(wavs)
            return [(np.full((80, 4), float(w.shape[0] % 7), dtype=np.float32), None) for w in wavs]

        def save(path, mel):
            with self.lock:
                self.events.append(("write_start", time.perf_counter(), path))
            np.save(path, mel)

        monkeypatch.setattr(preprocess, "read_wav", read_wav)
        monkeypatch.setattr(preprocess, "_save", save)
        self.run_batch = run_batch


def test_writes_start_before_the_corpus_is_decoded(tmp_path, monkeypatch):
    base = _tree(tmp_path)
    probe = _Probe(monkeypatch, run_s=0.02)
    out = tmp_path / "out"
    out.mkdir()
    st = preprocess.preprocess_vctk(base, out, batch_seconds=2.0, workers=4, run_batch=probe.run_batch)
    assert st["written"] == 40 and not st["skipped"]
    first_write = min(t for k, t, _ in probe.events if k == "write_start")
    last_decode = max(t for k, t, _ in probe.events if k == "decode_end")
    assert first_write < last_decode
    decoded_before_first_write = sum(1 for k, t, _ in probe.events if k == "decode_end" and t < first_write)
    assert decoded_before_first_write <= 4 * 4 + 2 + 1, decoded_before_first_write
    # held decodes: the window (4 x workers) plus the batch being filled (2 files of 1 s at 2 s per batch)
    assert probe.max_held <= 4 * 4 + 2 + 1, probe.max_held


def test_held_decodes_do_not_grow_with_the_corpus(tmp_path, monkeypatch):
    helds = []
    for n_utt in (10, 60):
        base = _tree(tmp_path / f"c{n_utt}", n_spk=1, n_utt=n_utt, seconds=0.25)
        probe = _Probe(monkeypatch, decode_s=0.001, run_s=0.02)
        out = tmp_path / f"o{n_utt}"
        out.mkdir()
        preprocess.preprocess_vctk(base, out, batch_seconds=1.0, workers=2, run_batch=probe.run_batch, decode_ahead=3)
        helds.append(probe.max_held)
    assert helds[1] <= 3 + 4 + 1, helds


def test_outputs_do_not_depend_on_batch_workers_or_window(tmp_path, monkeypatch):
    base = _tree(tmp_path, n_spk=2, n_utt=7, seconds=0.5)
    snaps = []
    for i, (bs, w, ahead) in enumerate(((0.4, 1, 1), (3.0, 16, None), (100.0, 3, 2))):
        probe = _Probe(monkeypatch, decode_s=0.0)
        out = tmp_path / f"o{i}"
        out.mkdir()
        preprocess.preprocess_vctk(base, out, batch_seconds=bs, workers=w, run_batch=probe.run_batch, decode_ahead=ahead)
        snaps.append({str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()})
    assert snaps[0] == snaps[1] == snaps[2]
    lines = snaps[0]["p225/_sources.txt"].decode().splitlines()
    assert [l.split(",")[0] for l in lines] == [f"p225_{u:03d}_mel.npy" for u in range(7)]
