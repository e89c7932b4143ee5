"""The float64 / integer restatement of the silence trimming of dvae_amd.preprocess (include/dvae_hip.h, "silence
trimming"; csrc/vad.hip), in numpy.  Not a test module: tests/test_vad_ref.py proves it on the CPU, tests/test_hip_vad.py
holds the kernels to it.

Per utterance y of n samples at 16 kHz, after volume normalisation:
  W = n // 480 windows; the tail of n % 480 samples is dropped
  E_w = sum over the window of (y[i] - 0.97 y[i-1])^2 in float64, y[-1] = 0 in front of the utterance only
  b_w = clamp(ilogb(E_w) + 80, 0, 95) from the double's exponent field (0 for zero and subnormals)
  b10, b90 = the smallest bins whose cumulative window count reaches ceil(W / 10), ceil(9 W / 10)
  t = max(66, min(b10 + 3, b90 - 5)); flag_w = b_w >= t
  mask_w = at least 5 of the 8 flags of [w - 3, w + 4]; keep_w = any mask of [w - 3, w + 3]; outside [0, W) both are 0
  dst_w = kept windows before w; K = kept windows; the output is the kept windows back to back.
The smoothing is the reference's (preprocessing/encoder/audio.py:100-115: a moving average of width 8 by cumsum, np.round,
binary_dilation with ones(6 + 1)) restated on integers; `smooth_by_formula` is that formula itself, for the comparison."""
import numpy as np

WINDOW, MA_WIDTH, MAX_SILENCE, PREEMPH = 480, 8, 6, 0.97
BINS, BIN_OFFSET, BIN_FLOOR, ABOVE_P10, BELOW_P90 = 96, 80, 66, 3, 5
TOO_SHORT, NO_SPEECH = "shorter than one 30 ms window", "no speech detected"


def energies(y):
    """y: fp32 or float64 samples -> E [W] float64 (numpy's pairwise sum per window: the order is the window's own)"""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    W = y.shape[0] // WINDOW
    y = y[:W * WINDOW]
    d = y - PREEMPH * np.concatenate([[0.0], y[:-1]])
    return np.sum((d * d).reshape(W, WINDOW), axis=1) if W else np.zeros(0)


def bins_of(E):
    """clamp(ilogb(E) + 80, 0, 95) from the exponent field; zero and subnormal E -> 0"""
    ex = ((np.ascontiguousarray(E, dtype=np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    return np.where(ex == 0, 0, np.clip(ex - 1023 + BIN_OFFSET, 0, BINS - 1)).astype(np.int32)


def threshold(b):
    """-> (b10, b90, t) of the bins of one utterance (any W >= 0)"""
    b = np.asarray(b, dtype=np.int64)
    W = b.shape[0]
    c = np.cumsum(np.bincount(b, minlength=BINS))
    b10 = int(np.argmax(c >= -(-W // 10)))
    b90 = int(np.argmax(c >= -(-9 * W // 10)))
    return b10, b90, max(BIN_FLOOR, min(b10 + ABOVE_P10, b90 - BELOW_P90))


def _window_counts(v, before, after):
    """per w: how many of v[w - before .. w + after] are set, zeros outside"""
    v = np.asarray(v, dtype=np.int64)
    c = np.concatenate([[0], np.cumsum(np.concatenate([np.zeros(before, np.int64), v, np.zeros(after, np.int64)]))])
    return c[before + after + 1:] - c[:len(v)]


def smooth(flags):
    """flags [W] of 0 / 1 -> (mask, keep) by the integer form"""
    flags = np.asarray(flags, dtype=np.int64)
    mask = (_window_counts(flags, 3, 4) >= 5).astype(np.int64)
    keep = (_window_counts(mask, 3, 3) >= 1).astype(np.int64)
    return mask, keep


def smooth_by_formula(flags):
    """the floating-point formula of audio.py:104-115 (needs scipy): the flags padded with (8 - 1) // 2 zeros in front and
    8 // 2 behind, running sums of 8 as differences of a float cumsum, divided by 8, np.round (half to even), then
    scipy's binary_dilation with ones(6 + 1)"""
    from scipy.ndimage import binary_dilation
    f = np.asarray(flags, dtype=np.float64)
    if f.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    run = np.cumsum(np.concatenate([np.zeros((MA_WIDTH - 1) // 2), f, np.zeros(MA_WIDTH // 2)]))
    sums = run[MA_WIDTH - 1:] - np.concatenate([[0.0], run[:-MA_WIDTH]])
    mask = np.round(sums / MA_WIDTH).astype(bool)
    keep = binary_dilation(mask, np.ones(MAX_SILENCE + 1))
    return mask.astype(np.int64), keep.astype(np.int64)


def detect(y):
    """-> dict(W, E, b, b10, b90, t, flags, mask, keep, dst, K) of one utterance"""
    E = energies(y)
    b = bins_of(E)
    b10, b90, t = threshold(b)
    flags = (b >= t).astype(np.int32)
    mask, keep = smooth(flags)
    keep = keep.astype(np.int32)
    dst = (np.cumsum(keep) - keep).astype(np.int32)
    return dict(W=len(E), E=E, b=b, b10=b10, b90=b90, t=t, flags=flags, mask=mask.astype(np.int32), keep=keep, dst=dst,
                K=int(keep.sum()))


def trim(y, r=None):
    """the kept windows of y back to back (y's dtype), 480 K samples"""
    y = np.asarray(y).reshape(-1)
    r = detect(y) if r is None else r
    W = r["W"]
    return y[:W * WINDOW].reshape(W, WINDOW)[r["keep"].astype(bool)].reshape(-1)


def skip_reason(y, r=None):
    r = detect(y) if r is None else r
    return TOO_SHORT if r["W"] == 0 else NO_SPEECH if r["K"] == 0 else None


def pow2_distance(E):
    """per window: the relative distance of E to the nearest power of two (inf for E == 0, whose bin is exact)"""
    E = np.asarray(E, dtype=np.float64)
    m, _ = np.frexp(E)                                 # E = m 2^e, m in [0.5, 1)
    return np.where(E > 0, np.minimum(m - 0.5, 1.0 - m) * 2.0, np.inf)


# ------------------------------------------------------------------------------------------------------ test utterances
FLOOR_DBFS = -62.0


def floor_noise(rs, n, dbfs=FLOOR_DBFS):
    """white noise of `dbfs` mean square"""
    return 10.0 ** (dbfs / 20.0) * rs.randn(n)


def burst(rs, n, f=220.0, amp=0.1):
    """a tone with a little noise: speech's stand-in, some 40 dB above the floor.  It ends in a ramp of 48 samples down
    to 0: cut off at full swing, its last sample would reach through the pre-emphasis into the first sample of the window
    behind it and flag that window too (a click is not silence)."""
    x = amp * np.sin(2 * np.pi * f * np.arange(n) / 16000.0 + 0.3) + 0.01 * rs.randn(n)
    m = min(48, n)
    x[n - m:] *= np.arange(m - 1, -1, -1) / 48.0
    return x


def utterance(rs, W, loud, tail=0, floor_dbfs=FLOOR_DBFS):
    """W windows + `tail` samples of floor noise with a burst over every window range [a, b) of `loud` -> fp32"""
    n = W * WINDOW + tail
    y = floor_noise(rs, n, floor_dbfs)
    for a, b in loud:
        y[a * WINDOW:b * WINDOW] += burst(rs, (b - a) * WINDOW)
    return y.astype(np.float32)


def expected_keep(W, loud):
    """What the rules keep when exactly the windows of `loud` are flagged."""
    flags = np.zeros(W, np.int64)
    for a, b in loud:
        flags[a:b] = 1
    return smooth(flags)[1]
