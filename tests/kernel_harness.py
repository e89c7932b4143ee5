"""What the kernel suites (tests/test_hip_*.py that hold a kernel family to a float64 reference through the C ABI) share on
the device side: the library handle, guarded buffers, bit comparisons and the worst error / bound table.  Not a test module:
tests/test_kernel_harness.py runs it on the CPU.  DESIGN.md section 5 describes it once for every family.

A launch may write only into a `Buf`: its payload lies in the middle of one uint8 allocation with at least PADB guard bytes
of 0xA5 on either side, and is filled with 0xFF before the launch, so an element the launch did not write is a NaN in fp32,
bf16 and fp64 and keeps the all-ones bits.  `guards` asserts after the launch that every guard byte kept its value.
"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)                    # the suites import dvae_amd and oracle from there
from ref_common import worst_ratio  # noqa: E402

DEV = "cuda"
EINVAL = -1
PADB = 256                                  # guard bytes on either side of every buffer, at least
GUARD = 0xA5
F32, F64 = np.float32, np.float64
TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint32): torch.int32}
BITS_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def L():
    from dvae_amd import _lib
    return _lib.lib()


def st():
    from dvae_amd import _lib
    return _lib.stream()


def sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def ok(rc, what=""):
    assert rc == 0, f"{what + ': ' if what else ''}return code {rc}, hipError {L().dvae_last_hip_error()}"


def down(t):
    sync()
    return t.cpu().numpy().copy()


def flat(opt):
    """p, g, m, v of a FlatAdam: its whole flat buffers as numpy."""
    return {k: down(getattr(opt, a)) for k, a in (("p", "flat_p"), ("g", "flat_g"), ("m", "exp_avg"), ("v", "exp_avg_sq"))}


def dev_equal(a, b):
    """Two tensors hold the same shape and the same bits (compared where they live)."""
    return a.shape == b.shape and bool(torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                   b.contiguous().reshape(-1).view(torch.uint8)))


class Buf:
    """A buffer of `shape` and `dtype` in the middle of one allocation with PADB (+ `lead` in front) guard bytes on either
    side; the payload is filled with `fill` bytes or with `data`.  `data` is a numpy array: its BITS are uploaded when its
    dtype is the buffer's, its values are converted otherwise (float64 -> fp32; bf16 from bf16-representable fp32 is exact).
    `shape` and `dtype` default to the data's (fp32 without data).  `lead` moves the payload to `lead` modulo 256 behind the
    allocation's start, for the kernels that choose a path from alignment.  `slack_from`: the payload bytes from there on
    (a workspace's tail that no kernel has a use for) must keep the fill, and count as guards."""

    def __init__(self, shape=None, dtype=None, data=None, fill=0xFF, lead=0, device="cuda"):
        if data is not None:
            data = np.ascontiguousarray(data)
            shape = data.shape if shape is None else shape
            dtype = TORCH_OF[data.dtype] if dtype is None else dtype
        self.shape, self.dtype = tuple(shape), torch.float32 if dtype is None else dtype
        self.fill, self.slack_from = fill, None
        self.esize = torch.empty((), dtype=self.dtype).element_size()
        self.nbytes = int(np.prod(self.shape)) * self.esize
        self.off = PADB + lead
        self.raw = torch.full((self.off + -(-self.nbytes // 16) * 16 + PADB,), GUARD, dtype=torch.uint8, device=device)
        inside = self.raw[self.off:self.off + self.nbytes]
        inside.fill_(fill)
        self.t = inside.view(self.dtype).view(self.shape)
        if data is not None and self.nbytes:
            if TORCH_OF.get(data.dtype) == self.dtype:
                inside.copy_(torch.from_numpy(data.reshape(-1).view(np.uint8)))
            else:
                self.t.copy_(torch.from_numpy(data).to(self.dtype).view(self.shape))
        assert self.ptr % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def at(self, k):
        """The address of element k of the flattened payload."""
        return self.ptr + k * self.esize

    def intact(self):
        sync()
        good = bool((self.raw[:self.off] == GUARD).all()) and bool((self.raw[self.off + self.nbytes:] == GUARD).all())
        if self.slack_from is not None:
            good = good and bool((self.raw[self.off + self.slack_from:self.off + self.nbytes] == self.fill).all())
        return good

    def np(self):
        """Values as numpy (bf16 widened exactly to fp32)."""
        sync()
        t = self.t.float() if self.dtype == torch.bfloat16 else self.t
        return t.cpu().numpy().copy()

    def bits(self):
        """The payload's bits as signed integers of the element's width."""
        sync()
        return self.t.view(BITS_OF[self.esize]).cpu().numpy().copy()

    def poisoned(self):
        """Per element: still the fill."""
        sync()
        return (self.t.contiguous().view(torch.uint8).view(*self.shape, self.esize) == self.fill).all(-1).cpu().numpy()


def P(b):
    return None if b is None else b.ptr


def guards(*bufs):
    for b in bufs:
        assert b is None or b.intact(), "a launch wrote outside its buffer"


class Pad:
    """An input of the launch: `data` (fp32) with `before` and `after` NaN elements around it in one guarded buffer;
    .ptr is the address of data[0]."""

    def __init__(self, data, before=4, after=64, device="cuda"):
        data = np.ascontiguousarray(data, F32)
        flat = np.concatenate([np.full(before, np.nan, F32), data.reshape(-1), np.full(after, np.nan, F32)])
        self.buf = Buf(data=flat, device=device)
        self.ptr = self.buf.at(before)


def ibuf(a, dtype=np.int64, device="cuda"):
    return Buf(data=np.ascontiguousarray(a, dtype), device=device)


def untouched(bits_, what):
    """`bits_` (Buf.bits() of fp32 elements, or a part of it) still holds the 0xFF fill."""
    assert (np.asarray(bits_).reshape(-1) == -1).all(), f"{what}: an element the launch must not write changed"


def bits(a):
    """The bits of fp32 values."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    """Predicate: two arrays of fp32 values have the same shape and the same bits."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def assert_same_bits(got, ref, what):
    """got: a Buf, or fp32 values downloaded from one; ref: fp32 values whose bits it must hold (flattened: only the size has
    to agree)."""
    g_, r_ = (got.bits().view(np.uint32) if isinstance(got, Buf) else bits(got)).reshape(-1), bits(ref).reshape(-1)
    assert g_.shape == r_.shape, f"{what}: {g_.size} elements instead of {r_.size}"
    bad = np.nonzero(g_ != r_)[0]
    assert not bad.size, (f"{what}: {bad.size} of {r_.size} elements differ in their bits, first at {bad[:1]}: "
                          f"{g_[bad[:1]].view(F32)} instead of {r_[bad[:1]].view(F32)}")


class Worst:
    """A module's table of the worst error / bound per key.  Keys are strings (printed on one line) or (row, column) pairs
    (printed as a table: rows sorted, columns in the order they first appeared)."""

    def __init__(self, title, sort=False, ratio_fn=worst_ratio):
        self.title, self.sort, self.ratio_fn, self.worst = title, sort, ratio_fn, {}

    def record(self, key, ratio):
        self.worst[key] = max(self.worst.get(key, 0.0), ratio)

    def note(self, key, got, ref, tol, what, skip=None, ratio_fn=None):
        """Record max |got - ref| / tol under `key` (elements where `skip` left out) and assert that it is at most 1."""
        got, ref = np.asarray(got, F64), np.asarray(ref, F64)
        tol = np.broadcast_to(tol, ref.shape)
        if skip is not None:
            keep = ~np.broadcast_to(skip, ref.shape)
            got, ref, tol = got[keep], ref[keep], tol[keep]
        r, i = (ratio_fn or self.ratio_fn)(got, ref, tol)
        self.record(key, r)
        assert r <= 1.0, (f"{what}: {key} at flat index {i}: {got.reshape(-1)[i]!r}, reference {ref.reshape(-1)[i]!r}, "
                          f"bound {tol.reshape(-1)[i]:.3g}, error / bound = {r:.3f}")
        return r

    def report(self):
        w = self.worst
        if not any(isinstance(k, tuple) for k in w):
            items = sorted(w.items()) if self.sort else w.items()
            print(f"\nworst error / bound over {self.title}: " + ", ".join(f"{k} {v:.3f}" for k, v in items))
            return
        cols = list(dict.fromkeys(c for _, c in w))
        print(f"\nworst error / bound over {self.title}\n| kernels | " + " | ".join(cols) + " |\n|---|" + "---|" * len(cols))
        for f in sorted({f for f, _ in w}):
            print(f"| {f} | " + " | ".join(f"{w[(f, c)]:.3f}" if (f, c) in w else "" for c in cols) + " |")


# ------------------------------------------------------------------ what the suites share above the kernels
def make_trainer(batch=4, n_frames=64, lr=1e-4):
    """The smallest trainer shape the trainer tests use, on deterministic weights."""
    import dvae_amd
    from oracle.fill import fill_state_dict
    w = dvae_amd.ConvolutionalMulVAE("VCTK", n_frames, 80, 32, lr, 0.01, 500, False, batch_size=batch, speaker_size=4,
                                     device=torch.device("cuda"), latent_dim=32, mse_cof=10, kl_cof=10)
    w.model.load_state_dict(fill_state_dict(w.model.state_dict()))
    w.model.train()
    return w


def child(module, argv, ok=True):
    """`python -m dvae_amd.train` / `dvae_amd.probe` with `argv` in a fresh child process, under a time limit."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    code = {"train": "import dvae_amd.train as t, sys; t.main(sys.argv[1:])",
            "probe": "import dvae_amd.probe as t, sys; sys.exit(t.main(sys.argv[1:]))"}[module]
    r = subprocess.run([sys.executable, "-c", code] + [str(a) for a in argv], env=env, capture_output=True, text=True, timeout=600)
    if ok:
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r
