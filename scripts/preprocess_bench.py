"""GPU box: corpus preprocessing (dvae_amd.preprocess) -- for a batch of 64 x 4 s utterances at 48 kHz and at 44.1 kHz the ms of
the resample kernel and of the volume kernels alone (tables prepared beforehand), of the pinned mel per call and of the whole
resample + normalise + mel path per call (host planning and table uploads included), files/s and peak resident memory of
the CLI end to end on a synthetic 48 kHz VCTK tree in a temporary directory (60 s batches: several of them), and the float64 numpy restatement (tests/test_preprocess.py) per second of 48 kHz audio.  Prints one JSON line."""
import json
import os
import resource
import subprocess
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import dvae_amd  # noqa: F401
from dvae_amd.frontend import MelFrontend
from dvae_amd.preprocess import Resampler, pack, volume_launch, volume_packed, volume_prepare


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def gpu_batch(sr, n_utt=64, seconds=4.0, reps=5):
    """kernel times on tables prepared beforehand (resample: dvae_resample_batch alone; volume: its three launches alone,
    each rep on a fresh copy of the resampled batch so that the gain pass is not skipped), and per-call times of the whole
    Python path (host planning, table uploads, allocations and the volume read-back included)"""
    rs = np.random.RandomState(0)
    xs = [(0.05 * rs.randn(int(sr * seconds))).astype(np.float32) for _ in range(n_utt)]
    fe, r = MelFrontend(), Resampler()
    x, _ = pack(xs)
    lens, srs = [len(a) for a in xs], [sr] * n_utt
    prep = r.prepare(lens, srs)
    table = prep["table"]
    y = r.launch(x, prep)
    y0 = y.clone()
    resample_kernel_ms = timed(lambda: r.launch(x, prep, y), reps)
    vprep = volume_prepare(table, y.device)
    copy_ms = timed(lambda: y.copy_(y0), reps)
    volume_kernel_ms = timed(lambda: (y.copy_(y0), volume_launch(y, vprep)), reps) - copy_ms
    mel_call_ms = timed(lambda: fe.mel_packed(y0, table[:, 2], table[:, 3]), reps)

    def whole():
        yy, tt = r.packed(x, lens, srs)
        volume_packed(yy, tt)
        fe.mel_packed(yy, tt[:, 2], tt[:, 3])
    call_ms = timed(whole, reps)
    taps = r._rows[r._ids[sr]][2]
    fma = float(table[:, 4].sum()) * taps
    return dict(ms_per_call=round(call_ms, 3), resample_kernel_ms=round(resample_kernel_ms, 3),
                volume_kernels_ms=round(volume_kernel_ms, 3), mel_ms_per_call=round(mel_call_ms, 3), taps=int(taps),
                resample_kernel_tflops=round(2 * fma / resample_kernel_ms / 1e9, 2))


def cli_files_per_s(n_spk=4, n_utt=32, seconds=3.0):
    rs = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as d:
        for s in range(n_spk):
            sd = os.path.join(d, "VCTK-Corpus", "wav16", f"p{225 + s}")
            os.makedirs(sd)
            for u in range(n_utt):
                v = np.clip(rs.randn(int(48000 * seconds)) * 3000, -32768, 32767).astype("<i2")
                with wave.open(os.path.join(sd, f"p{225 + s}_{u:03d}.wav"), "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(48000)
                    w.writeframes(v.tobytes())
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        t0 = time.perf_counter()
        subprocess.run([sys.executable, "-m", "dvae_amd.preprocess", d, "-o", os.path.join(d, "out"), "--no_trim",
                        "--batch-seconds", "60"], env=env, check=True, capture_output=True, timeout=600)
        dt = time.perf_counter() - t0
    peak_mb = resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss / 1024.0
    return round(n_spk * n_utt / dt, 1), round(dt, 2), round(peak_mb)


def main():
    from test_preprocess import normalize_ref, resample_ref
    res = dict(utterances=64, seconds=4.0)
    res["sr48000"] = gpu_batch(48000)
    res["sr44100"] = gpu_batch(44100)
    x = (0.05 * np.random.RandomState(2).randn(48000)).astype(np.float32)
    t0 = time.perf_counter()
    normalize_ref(resample_ref(x, 48000))
    res["cpu_fp64_ms_per_audio_second"] = round(1e3 * (time.perf_counter() - t0), 1)
    res["cli_files_per_s"], res["cli_wall_s_128_files_3s"], res["cli_peak_rss_mb"] = cli_files_per_s()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
