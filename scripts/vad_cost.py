"""GPU box: what silence trimming costs (dvae_amd.preprocess --trim, csrc/vad.hip) beside the volume pass that reads the same
bytes.  Per launch of dvae_volume_normalize and dvae_vad_trim, timed with device events on the launch stream (the library's
opt-in family DVAE_PROF_AUDIO), in one process: 3 warm-up calls, then the minimum and median of 10, on 64 x 4 s and on one
600 s utterance at 16 kHz; GB/s over each launch's algorithmic bytes (sum of squares and window energies: 4 B per sample
read; compaction: 4 B read and 4 B written per kept sample; the volume gain pass: 4 B read and 4 B written per sample).
Then the wall time of the CLI on a synthetic 48 kHz tree with --trim and with --no_trim.  Prints one JSON line and the
line of the `vad_cost` block of README.md / DESIGN.md section 4.5."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import dvae_amd  # noqa: F401
from dvae_amd._lib import lib
from dvae_amd.preprocess import VAD_WINDOW, pack, vad_launch, vad_prepare, volume_launch, volume_prepare

PROF_AUDIO = 3                                          # DVAE_PROF_AUDIO
TAGS = {0: "sumsq", 1: "volume_finalize", 2: "volume_scale", 3: "vad_energy", 4: "vad_mask", 5: "vad_compact"}
WARMUP, CALLS = 3, 10


def speech_like(rs, seconds):
    """a -62 dBFS floor with tone-plus-noise speech over the middle 60 % and a pause inside it"""
    n = int(16000 * seconds)
    y = 10.0 ** (-62 / 20.0) * rs.randn(n)
    a, b = int(0.2 * n), int(0.8 * n)
    y[a:b] += 0.1 * np.sin(2 * np.pi * 220.0 * np.arange(b - a) / 16000.0) + 0.01 * rs.randn(b - a)
    p = (a + b) // 2
    y[p:p + min(16000, (b - a) // 4)] *= 1e-3
    return (0.2 * y).astype(np.float32)                  # under -30 dBFS: the gain pass has work to do


def per_launch(utterances):
    L = lib()
    y0, offs = pack(utterances)
    table = np.zeros((len(utterances), 6), np.int64)
    table[:, 2], table[:, 3] = offs, [len(u) for u in utterances]
    y, out = y0.clone(), torch.empty_like(y0)
    vol, vad = volume_prepare(table, y.device), vad_prepare(table, y.device)
    tags, ms = (C.c_uint * 8)(), (C.c_double * 8)()
    launches, flops, nbytes = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_double * 8)()
    seen = {t: [] for t in TAGS}
    for call in range(WARMUP + CALLS):
        y.copy_(y0)
        torch.cuda.synchronize()
        L.dvae_prof_enable(PROF_AUDIO)
        volume_launch(y, vol)
        vad_launch(y, vad, out)
        n = L.dvae_prof_collect_tags(tags, ms, launches, flops, nbytes, 8)
        L.dvae_prof_collect(None, None, None)
        L.dvae_prof_enable(0)
        assert n == len(TAGS) and all(launches[i] == 1 for i in range(n)), (n, list(launches))
        if call >= WARMUP:
            for i in range(n):
                seen[tags[i]].append(ms[i] * 1e3)
    samples = int(table[:, 3].sum())
    kept = VAD_WINDOW * int(vad["K"].sum().item())
    alg = {0: 4 * samples, 2: 8 * samples, 3: 4 * VAD_WINDOW * vad["nwin"], 5: 8 * kept}
    res = dict(samples=samples, windows=vad["nwin"], kept_samples=kept)
    for t, name in TAGS.items():
        us = sorted(seen[t])
        res[name] = dict(min_us=round(us[0], 1), median_us=round(float(np.median(us)), 1))
        if t in alg:
            res[name]["GBps_at_min"] = round(alg[t] / us[0] / 1e3, 1)
    return res


def cli_wall(n_spk=4, n_utt=16, seconds=3.0):
    rs = np.random.RandomState(1)
    with tempfile.TemporaryDirectory() as d:
        for s in range(n_spk):
            sd = os.path.join(d, "VCTK-Corpus", "wav16", f"p{225 + s}")
            os.makedirs(sd)
            for u in range(n_utt):
                x = np.repeat(speech_like(rs, seconds), 3)                   # 48 kHz by repetition: the timing's input only
                with wave.open(os.path.join(sd, f"p{225 + s}_{u:03d}.wav"), "wb") as w:
                    w.setnchannels(1)
                    w.setsampwidth(2)
                    w.setframerate(48000)
                    w.writeframes(np.clip(np.round(x * 32767), -32768, 32767).astype("<i2").tobytes())
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        wall = {}
        for flag in ("--no_trim", "--trim"):
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, "-m", "dvae_amd.preprocess", d, "-o", os.path.join(d, "out" + flag), flag],
                               env=env, check=True, capture_output=True, text=True, timeout=600)
            wall[flag] = round(time.perf_counter() - t0, 2)
            wall[flag + "_summary"] = r.stdout.strip().splitlines()[-1][:120]
    return dict(files=n_spk * n_utt, seconds_each=seconds, **wall)


def main():
    rs = np.random.RandomState(0)
    res = dict(device=torch.cuda.get_device_name(0), calls=CALLS)
    res["64x4s"] = per_launch([speech_like(rs, 4.0) for _ in range(64)])
    res["1x600s"] = per_launch([speech_like(rs, 600.0)])
    res["cli"] = cli_wall()
    print(json.dumps(res))
    cell = lambda r, k: f"{r[k]['min_us']} / {r[k]['median_us']} µs" + (f" ({r[k]['GBps_at_min']} GB/s)" if "GBps_at_min" in r[k] else "")
    for name in ("64x4s", "1x600s"):
        print(f"{name}: " + "; ".join(f"{k} {cell(res[name], k)}" for k in TAGS.values()))


if __name__ == "__main__":
    main()
