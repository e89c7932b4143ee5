"""The LSTM recurrence kernels on the MI355X (csrc/lstm.hip, csrc/lstm_pers.hip) against the float64 reference of
tests/lstm_ref.py, frame by frame, through the C ABI (dvae_lstm_seq_fwd / _bwd / _fwd_range / _bwd_range).

Every comparison is ONE FRAME judged from the device's own neighbours: a whole-sequence launch (H = 64, generic H, the
persistent launches) is downloaded once and every frame is recomputed in float64 from what the device stored for the frame
before it (h, c; in the backward pass its own gates, c_all and dgates of the frame after it); the per-frame kernels of
H % 512 == 0 are stepped through dvae_lstm_seq_bwd_range and dc_ws is read after every step.  The bounds are those derived
in tests/lstm_ref.py, per element, never a fraction of a tensor's maximum; 100 % of the elements are compared.  The cases
are `lstm_ref.CASES`: tests/test_lstm_ref.py asserts which kernel each of them reaches.

Every buffer a launch may write is a guarded one of tests/kernel_harness.py.  Where two directions write columns of one
tensor, one direction is also run alone and the other one's columns must keep their poison.  A bf16-stored h or dG is held
through its bound and, besides, to the same case run with fp32 storage (2^-8 relative plus the fp32 bound: in the bf16
mode both runs feed the next frame the same rounded operand).  The whole-sequence kernels (H = 64, persistent) keep the
cell-gradient carry in registers and never store dc_ws: there it must keep its poison.  The worst error / bound per kernel
family and quantity is printed at the module's end.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
from kernel_harness import Buf, DEV, guards, L, Worst      # first: it puts the repository root on sys.path
import dvae_amd  # noqa: E402,F401
from dvae_amd import _lib, ops  # noqa: E402
from dvae_amd.derived import lstm_local  # noqa: E402
import lstm_ref as R  # noqa: E402

WORST = Worst("test_hip_lstm.py")              # (kernel family, quantity) -> worst error / bound over this module
FP32_STORED = {}                            # case with fp32 storage -> per entry (h, dG, their bounds): the bf16-stored twin reads it


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    WORST.report()


def note(fam, res, what):
    for k, (r, where) in res.items():
        WORST.record((fam, k), r)
    for k, (r, where) in res.items():
        assert r <= 1.0, f"{what}: {k}: error / bound = {r:.3f} at {where}"


def family(c, bmode=None):
    m = R.MODE_NAMES[c.mode] + ("/bf16 state" if c.st16 else "")
    return f"{c.fam} {m}" if bmode is None or bmode == c.mode else f"{c.fam} {m}, backward {R.MODE_NAMES[bmode]}"


class Layer:
    """The inputs and weight-derived operands of every entry of a case on the device, and its forward pass."""

    def __init__(self, c):
        self.c, self.n = c, len(c.rev)
        T, N, H = c.T, c.N, c.H
        self.ent = R.make_inputs(c)
        self.sdt = torch.bfloat16 if c.st16 else torch.float32
        f = dict(device=DEV, dtype=torch.float32)
        self.w = [torch.from_numpy(e["W"]).to(DEV) for e in self.ent]
        zb = torch.zeros(4 * H, **f)
        self.der = [lstm_local(torch.zeros(4 * H, 64, **f), w, zb, zb, c.mode) for w in self.w]
        self.ldh = 2 * H if c.ldh2 else H
        self.ldg = 8 * H if c.gld2 else 4 * H
        self.cbuf = [Buf((T, N, H)) for _ in range(self.n)]
        self.gates, self.gptr = self.shared(c.gld2, 4 * H, torch.float32, "x")
        self.h, self.hptr = self.shared(c.ldh2, H, self.sdt, None)
        self.forward()

    def shared(self, side_by_side, width, dtype, key):
        """One buffer per entry, or both directions' columns side by side in one; (buffers, pointer per entry)."""
        T, N = self.c.T, self.c.N
        data = [e[key] for e in self.ent] if key else None
        if side_by_side:
            assert self.n == 2
            b = Buf((T, N, 2 * width), dtype, None if data is None else np.concatenate(data, 2))
            return [b], [b.ptr, b.at(width)]
        bufs = [Buf((T, N, width), dtype, None if data is None else data[i]) for i in range(self.n)]
        return bufs, [b.ptr for b in bufs]

    def cols(self, bufs, side_by_side, width, i):
        """Entry i's [T, N, width] of what `shared` made, as numpy."""
        return bufs[0].np()[:, :, i * width:(i + 1) * width] if side_by_side else bufs[i].np()

    def fwd_dirs(self, gptr, hptr, which, pers):
        c = self.c
        d = (_lib.LstmDir * len(which))()
        for k, i in enumerate(which):
            d[k].gates, d[k].w_hh, d[k].h_out, d[k].c_all = gptr[i], _lib.ptr(self.w[i]), hptr[i], self.cbuf[i].ptr
            d[k].w_packed = _lib.ptr(self.der[i].pack_f)
            d[k].reverse, d[k].packed_mode, d[k].step_shift, d[k].state_bf16 = c.rev[i], c.mode, c.shifts[i], c.st16
            d[k].gate_ld = self.ldg if c.gld2 else 0
            if pers:
                d[k].pers_ws = _lib.ptr(ops.lstm_pers_workspace(DEV))
        return d

    def forward(self):
        c = self.c
        T, N, H = c.T, c.N, c.H
        pers = c.fam == "pers"
        if pers:
            assert L().dvae_lstm_pers_supported(N, H, c.mode, 0) == 1, "no persistent forward launch for this case"
            assert 0 < L().dvae_lstm_pers_ws_bytes(N, H) <= ops.lstm_pers_workspace(DEV).numel()
        d = self.fwd_dirs(self.gptr, self.hptr, range(self.n), pers)
        if any(c.shifts):
            rc = L().dvae_lstm_seq_fwd_range(d, self.n, T, N, H, self.ldh, 0, T + max(c.shifts), _lib.stream())
        else:
            rc = L().dvae_lstm_seq_fwd(d, self.n, T, N, H, self.ldh, _lib.stream())
        assert rc == 0, rc
        if pers:
            ops.lstm_pers_check()
        guards(*self.gates, *self.h, *self.cbuf)
        self.dev = [{"gates": self.cols(self.gates, c.gld2, 4 * H, i), "c": self.cbuf[i].np(),
                     "h": self.cols(self.h, c.ldh2, H, i)} for i in range(self.n)]

    def backward(self, bmode, stepped, pers, bias):
        """One backward pass in arithmetic `bmode`.  Returns per entry (dG, last dc_ws or None, dc_ws after every step or
        None, bias buffers)."""
        c = self.c
        T, N, H = c.T, c.N, c.H
        g16 = bool(c.st16) and bmode == R.MODE_BF16
        gdt = torch.bfloat16 if g16 else torch.float32
        if c.ldh2:
            dh = torch.from_numpy(np.concatenate([e["dh"] for e in self.ent], 2)).to(DEV)
            dhptr = [dh.data_ptr(), dh.data_ptr() + 4 * H]
        else:
            dh = [torch.from_numpy(e["dh"]).to(DEV) for e in self.ent]
            dhptr = [t.data_ptr() for t in dh]
        dg, dgptr = self.shared(c.gld2, 4 * H, gdt, None)
        dc = [Buf((N, H)) for _ in range(self.n)]
        packs = [self.der[i].pack_b for i in range(self.n)]
        if bmode != c.mode:                         # fp32 fragments of W_hh for a backward pass after an fp32x3 forward pass
            assert bmode == R.MODE_F32
            packs = [torch.empty(4 * H * H, device=DEV, dtype=torch.float32) for _ in range(self.n)]
            for i in range(self.n):
                assert L().dvae_lstm_pack_w(_lib.ptr(self.w[i]), None, _lib.ptr(packs[i]), H, _lib.stream()) == 0
        db = dbp = None
        if bias == "ih_hh":
            db = Buf((2, 4 * H), torch.float32, self.ent[0]["db0"])
        elif bias == "part":
            dbp = Buf((_lib.PERS_BIAS_SLABS, 4 * H))
        d = (_lib.LstmDir * self.n)()
        for i in range(self.n):
            d[i].gates, d[i].c_all, d[i].w_hh, d[i].w_packed = self.gptr[i], self.cbuf[i].ptr, _lib.ptr(self.der[i].w_hh_t), _lib.ptr(packs[i])
            d[i].dh_out, d[i].dgates, d[i].dc_ws = dhptr[i], dgptr[i], dc[i].ptr
            d[i].reverse, d[i].packed_mode, d[i].step_shift, d[i].state_bf16 = c.rev[i], bmode, c.shifts[i], int(g16)
            d[i].gate_ld = self.ldg if c.gld2 else 0
            if pers:
                d[i].pers_ws = _lib.ptr(ops.lstm_pers_workspace(DEV))
                if db is not None:
                    d[i].dbias_ih, d[i].dbias_hh = db.ptr, db.at(4 * H)
                if dbp is not None:
                    d[i].dbias_part = dbp.ptr
        steps = None
        if stepped:
            steps = [[] for _ in range(self.n)]
            for s in range(T + max(c.shifts)):
                assert L().dvae_lstm_seq_bwd_range(d, self.n, T, N, H, self.ldh, s, s + 1, _lib.stream()) == 0
                for i in range(self.n):
                    if 0 <= s - c.shifts[i] < T:
                        steps[i].append(dc[i].np())
        else:
            if pers:
                assert L().dvae_lstm_pers_supported(N, H, bmode, 1) == 1, "no persistent backward launch for this case"
            assert L().dvae_lstm_seq_bwd(d, self.n, T, N, H, self.ldh, _lib.stream()) == 0
            if pers:
                ops.lstm_pers_check()
        guards(*dg, *dc, db, dbp, *self.gates, *self.cbuf)
        out = []
        for i in range(self.n):
            dG = self.cols(dg, c.gld2, 4 * H, i)
            assert np.isfinite(dG).all(), "dgates not finite"
            out.append((dG, dc[i], None if steps is None else steps[i], db, dbp))
        return out


def judge_backward(lay, bmode, stepped, pers, bias, what, tols=None):
    """tols: per entry, a dictionary that receives dG and its bounds."""
    c = lay.c
    g16 = bool(c.st16) and bmode == R.MODE_BF16
    for i, (dG, dc, steps, db, dbp) in enumerate(lay.backward(bmode, stepped, pers, bias)):
        if tols is not None:
            tols[i]["dG"] = dG
        e = lay.ent[i]
        dev = dict(lay.dev[i], dG=dG)
        if c.fam in ("gen", "v5"):
            dev["dc"] = dc.np()                   # the per-frame kernels leave the carry of the last step in dc_ws
        else:
            assert dc.poisoned().all(), "a whole-sequence kernel keeps the carry in registers: dc_ws is not touched"
        res = R.check_dir(e["x"], e["W"], e["dh"], c.rev[i], bmode, dev, g_bf16=g16, dc_steps=steps, passes="b",
                          tols=None if tols is None else tols[i])
        if db is not None:
            both = db.np()
            for k, name in enumerate(("dbias_ih", "dbias_hh")):
                r, j = R.bias_check(dG, e["db0"][k], both[k])["dbias"]
                if r >= res.get("dbias", (-1.0, ""))[0]:
                    res["dbias"] = (r, f"{name} column {j}")
        if dbp is not None:
            assert not dbp.poisoned().any(), "dbias_part: every slab is written"
            res.update({k: (r, f"column {j}") for k, (r, j) in R.bias_check(dG, None, None, slabs=dbp.np()).items()})
        note(family(c, bmode), res, f"{what} entry {i} backward {R.MODE_NAMES[bmode]} {bias or ''}")


def judge_case(c):
    """Forward and backward passes of a case, every frame judged.  Returns the layer and per entry {h, dG, tol_h, tol_dG}."""
    what = R.case_id(c) + " (" + c.note + ")"
    lay = Layer(c)
    tols = [{} for _ in lay.ent]
    for i, e in enumerate(lay.ent):
        assert not any(np.isnan(lay.dev[i][k]).any() for k in ("gates", "c", "h")), f"{what}: an element was not written"
        res = R.check_dir(e["x"], e["W"], e["dh"], c.rev[i], c.mode, lay.dev[i], h_bf16=bool(c.st16), passes="f", tols=tols[i])
        tols[i]["h"] = lay.dev[i]["h"]
        note(family(c), res, f"{what} entry {i} forward")
    if c.fam == "pers":
        for bmode in c.bwd:
            for bias in ("ih_hh", "part"):
                judge_backward(lay, bmode, False, True, bias, what, tols if bmode == c.mode else None)
    else:
        judge_backward(lay, c.mode, c.fam == "v5", False, None, what, tols)
    return lay, tols


@pytest.mark.parametrize("case", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_every_frame_follows_from_the_devices_own_neighbours(case):
    c = case
    T, N, H = c.T, c.N, c.H
    what = R.case_id(c) + " (" + c.note + ")"
    lay, tols = judge_case(c)
    if c.mode == R.MODE_BF16 and c.fam != "h64" and not c.st16:
        FP32_STORED[c] = tols
    if c.st16:
        # the same case with fp32 storage of h and dG (run here where it is no case of its own)
        twin = c._replace(st16=0)
        if twin not in FP32_STORED:
            FP32_STORED[twin] = judge_case(twin)[1]
        for i, (t16, t32) in enumerate(zip(tols, FP32_STORED[twin])):
            res = {}
            for k in ("h", "dG"):
                tol32 = np.stack([t32["tol_" + k][t] for t in range(T)])
                r, j = R.stored_bf16_check(t16[k], t32[k], tol32)
                res[k + " bf16 vs fp32 storage"] = (r, f"flat index {j}")
            print(f"{what} entry {i}: " + ", ".join(f"{k} {r:.3f}" for k, (r, _) in res.items()))
            note(family(c), res, f"{what} entry {i}")
    if c.ldh2 or c.gld2:
        # the second direction alone into fresh tensors: the first one's columns keep their poison
        g2, gp2 = lay.shared(c.gld2, 4 * H, torch.float32, "x")
        h2, hp2 = lay.shared(c.ldh2, H, lay.sdt, None)
        c2 = Buf((T, N, H))
        keep = lay.cbuf[1]
        lay.cbuf[1] = c2
        d = lay.fwd_dirs(gp2, hp2, [1], False)
        assert L().dvae_lstm_seq_fwd(d, 1, T, N, H, lay.ldh, _lib.stream()) == 0
        lay.cbuf[1] = keep
        guards(*g2, *h2, c2)
        if c.ldh2:
            p = h2[0].poisoned()
            assert p[:, :, :H].all() and not p[:, :, H:].any(), "one direction alone touched the other one's columns of h_out"
        if c.gld2:
            g = g2[0].np()
            assert np.array_equal(g[:, :, :4 * H], lay.ent[0]["x"]), "one direction alone touched the other one's gates"
        e = lay.ent[1]
        dev = {"gates": lay.cols(g2, c.gld2, 4 * H, 1), "c": c2.np(), "h": lay.cols(h2, c.ldh2, H, 1)}
        note(family(c), R.check_dir(e["x"], e["W"], e["dh"], c.rev[1], c.mode, dev, h_bf16=bool(c.st16), passes="f"),
             f"{what} second direction alone")
