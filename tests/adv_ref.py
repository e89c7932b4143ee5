"""Float64 numpy restatement of the speaker adversary's two launches (dvae_adv_rows, dvae_adv_params; csrc/adversary.hip,
DESIGN.md section 4.18), the error bounds the kernels are held to, an fp32 walk in the kernels' own order, and the seeded
inputs of the GPU cases.  Not a test module: tests/test_adv_ref.py, tests/test_hip_adversary.py and
tests/test_hip_adversary_train.py use it.  Shapes: x [R, D] (dense: the caller cuts the columns out), labels [R], w1 [H, D]
(without padding), b1 [H], w2 [S, H], b2 [S]; lam and inv_rows are the fp32 values the device holds, as float64.

The bounds (EPS32 = 2^-24 is one rounding, g(k) = k EPS32 / (1 - k EPS32) is k of them compounded; |.| of a sum is the sum
of the absolute terms; E. is the bound of the stage before; every sum is taken in the kernel's order, whose DEPTH — the
roundings one term can pass through — is what g counts):

pre, h      D fmas in a chain and the bias: g(D + 1) (|w1| |x| + |b1|).  relu keeps it where pre can be positive.
logit       lane l adds 4 ceil(H / 256) terms in a chain, the xor tree adds 6 levels, then the bias: n_B = 4 ceil(H / 256) + 7
            roundings, g(n_B) (|w2| (|h| + Eh) + |b2|), and the data |w2| Eh.
softmax     d = logit - max: both logits' bounds and one rounding.  expf is within 1 ulp = 2 EPS32 of exp on its fp32 argument:
            e is off by the factor exp(+-Ed) (1 +- 2 EPS32).  s: lane chains of ceil(S / 64) terms and 6 levels.
            1 / s: the sum's relative bound and 2 EPS32.  p = e (1 / s): one more rounding; p - onehot: one; times inv_rows: one.
            A flushed denormal is below FLOOR = 2^-126 beside s >= 1.
loss        logf is within 1 ulp of ln s on the fp32 s: -log1p(-Es / s) + 2 EPS32 ln s, the label's d, one rounding.
g1          S fmas in a chain: |w2|^T Eg2 + g(S) |w2|^T (|g2| + Eg2), where h > 0; exactly 0 elsewhere.
dx          runs of H / 8 fmas, 7 additions, the product with lambda: g(H / 8 + 8) on the absolute terms, and the data.
params      R fmas (additions) in a chain: g(R) on the absolute terms, and the data of both factors.
out         float64 sums of the fp32 row losses (R EPS64 on the absolute terms), rounded once to fp32.
"""
import numpy as np

from ref_common import EPS32, EPS64, F, F64, FLOOR, fma, g

MAX_D, MAX_H, MAX_S = 64, 1024, 1024          # DVAE_ADV_MAX_D, DVAE_ADV_MAX_H, DVAE_CE_MAX_CLASSES
NW = 8                                        # runs of the dx sum (waves of a row's workgroup)
MARGIN = 10.0                                 # the GPU cases keep every pre-activation and top-two gap this many bounds away

# the GPU cases of tests/test_hip_adversary.py: (R, D, H, S) and what is special about each
CASES = {
    "one":    dict(shape=(1, 1, 64, 2), seed=11),
    "small":  dict(shape=(3, 5, 64, 5), seed=12, ldx_extra=3, col0=2),          # ldx > D: x is a block of a wider table
    "odd":    dict(shape=(5, 28, 128, 109), seed=13, ignored={1: -1, 3: 109}),   # a negative label and a label >= S
    "step":   dict(shape=(128, 28, 256, 109), seed=14),                          # the training step's shape
    "limits": dict(shape=(130, 64, 1024, 1024), seed=15),
}


def counted_rows(labels, S):
    labels = np.asarray(labels)
    return (labels >= 0) & (labels < S)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def rows64(x, labels, w1, b1, w2, b2, lam, inv_rows):
    """dvae_adv_rows in float64 -> dict(pre, h, logit, loss, pred, g2, g1, dx, counted)"""
    x, w1, b1, w2, b2 = (np.asarray(v, F64) for v in (x, w1, b1, w2, b2))
    labels = np.asarray(labels, np.int64)
    R, S = x.shape[0], w2.shape[0]
    cnt = counted_rows(labels, S)
    pre = x @ w1.T + b1
    h = np.where(pre > 0, pre, 0.0)
    logit = h @ w2.T + b2
    m = logit.max(axis=1, keepdims=True)
    e = np.exp(logit - m)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    onehot = np.zeros((R, S))
    onehot[np.nonzero(cnt)[0], labels[cnt]] = 1.0
    lab = np.where(cnt, labels, 0)
    loss = np.where(cnt, np.log(s[:, 0]) - (logit[np.arange(R), lab] - m[:, 0]), 0.0)
    g2 = np.where(cnt[:, None], float(inv_rows) * (p - onehot), 0.0)
    g1 = np.where(h > 0, g2 @ w2, 0.0)
    dx = -(float(lam) * (g1 @ w1))
    if float(lam) == 0.0:
        dx = np.zeros_like(dx)
    dx = np.where(cnt[:, None], dx, 0.0)
    return dict(pre=pre, h=h, logit=logit, loss=loss, pred=logit.argmax(axis=1), g2=g2, g1=g1, dx=dx, counted=cnt,
                e=e, s=s[:, 0], p=p, onehot=onehot, m=m[:, 0])


def params64(x, labels, res, inv_rows):
    """dvae_adv_params in float64 on the float64 rows -> dict(dw1, db1, dw2, db2, out)"""
    x = np.asarray(x, F64)
    cnt = res["counted"]
    g2, g1, h = res["g2"][cnt], res["g1"][cnt], res["h"][cnt]
    tot = float(res["loss"][cnt].sum())
    hits = int((res["pred"][cnt] == np.asarray(labels)[cnt]).sum())
    return dict(dw2=g2.T @ h, db2=g2.sum(axis=0), dw1=g1.T @ x[cnt], db1=g1.sum(axis=0),
                out=np.array([tot, float(cnt.sum()), float(hits), tot * float(inv_rows)]))


# ----------------------------------------------------------------------------------------------------------- the bounds
def bounds(x, labels, w1, b1, w2, b2, lam, inv_rows, res=None):
    """elementwise bounds of every output of the two launches against rows64 / params64 -> dict keyed like theirs (pred and
    the counts are exact), plus `pre` and `logit` (the margins of the GPU cases are measured in them)"""
    x, w1, b1, w2, b2 = (np.asarray(v, F64) for v in (x, w1, b1, w2, b2))
    res = rows64(x, labels, w1, b1, w2, b2, lam, inv_rows) if res is None else res
    R, D = x.shape
    H, S = w1.shape[0], w2.shape[0]
    u, ir, al = EPS32, float(inv_rows), abs(float(lam))
    ax, aw1, aw2 = np.abs(x), np.abs(w1), np.abs(w2)
    cnt = res["counted"]
    Epre = g(D + 1) * (ax @ aw1.T + np.abs(b1)) + FLOOR
    Eh = np.where(res["pre"] > -Epre, Epre, FLOOR)        # (FLOOR where a value is exactly 0: 0 / 0 is no ratio)
    ah = np.abs(res["h"]) + Eh
    nB = 4 * -(-H // 256) + 7
    Elog = Eh @ aw2.T + g(nB) * (ah @ aw2.T + np.abs(b2)) + FLOOR
    am = res["logit"].argmax(axis=1)
    d = res["logit"] - res["m"][:, None]
    Ed = (Elog + Elog[np.arange(R), am][:, None]) * (1 + u) + u * np.abs(d)
    rel_e = np.expm1(Ed) * (1 + 2 * u) + 2 * u
    e, s, p = res["e"], res["s"][:, None], res["p"]
    Ee = e * rel_e + FLOOR
    Es = Ee.sum(axis=1, keepdims=True) + g(-(-S // 64) + 6) * (e + Ee).sum(axis=1, keepdims=True)
    rel_s = Es / s
    rel_inv = rel_s / (1 - rel_s) + 2 * u
    Ep = p * ((1 + rel_e) * (1 + rel_inv) * (1 + u) - 1) + FLOOR
    t = p - res["onehot"]
    Et = Ep + u * (np.abs(t) + Ep)
    Eg2 = np.where(cnt[:, None], ir * Et * (1 + u) + u * np.abs(res["g2"]) + FLOOR, FLOOR)
    lab = np.where(cnt, np.asarray(labels, np.int64), 0)
    ln_s = np.log(res["s"])
    Eloss = (-np.log1p(-rel_s[:, 0]) + 2 * u * (ln_s + rel_s[:, 0]) + Ed[np.arange(R), lab]) * (1 + u) + u * np.abs(res["loss"]) + FLOOR
    Eloss = np.where(cnt, Eloss, FLOOR)
    ag2 = np.abs(res["g2"]) + Eg2
    Eg1 = np.where(res["h"] > 0, Eg2 @ aw2 + g(S) * (ag2 @ aw2) + FLOOR, FLOOR)
    # a unit whose pre-activation could take either sign may be gated the other way: all of g1 there
    Eg1 = np.where(np.abs(res["pre"]) <= Epre, np.abs(ag2 @ aw2) * (1 + g(S)) + FLOOR, Eg1)
    ag1 = np.abs(res["g1"]) + Eg1
    if float(lam) == 0.0:
        Edx = np.full((R, D), FLOOR)
    else:
        Edx = al * (Eg1 @ aw1 + g(H // NW + 8) * (ag1 @ aw1)) * (1 + u) + u * np.abs(res["dx"]) + FLOOR
        Edx = np.where(cnt[:, None], Edx, FLOOR)
    c = cnt
    out = dict(pre=Epre, h=Eh, logit=Elog, loss=Eloss, g2=Eg2, g1=Eg1, dx=Edx)
    out["dw2"] = Eg2[c].T @ ah[c] + np.abs(res["g2"][c]).T @ Eh[c] + g(R) * (ag2[c].T @ ah[c]) + FLOOR
    out["db2"] = Eg2[c].sum(axis=0) + g(R) * ag2[c].sum(axis=0) + FLOOR
    out["dw1"] = Eg1[c].T @ ax[c] + g(R) * (ag1[c].T @ ax[c]) + FLOOR
    out["db1"] = Eg1[c].sum(axis=0) + g(R) * ag1[c].sum(axis=0) + FLOOR
    tot, sl, sa = float(res["loss"][c].sum()), float(Eloss.sum()), float(np.abs(res["loss"][c]).sum())
    e0 = sl + R * EPS64 * (sa + sl) + u * (abs(tot) + sl) + FLOOR
    e3 = (sl + R * EPS64 * (sa + sl)) * ir * (1 + u) + u * (abs(tot) * ir + sl * ir) + FLOOR
    out["out"] = np.array([e0, 0.0, 0.0, e3])
    return out


def margins(res, bnd):
    """per row: the smallest |pre| / bound over the hidden units, and the top-two logit gap over the sum of their bounds"""
    pre = (np.abs(res["pre"]) / bnd["pre"]).min(axis=1)
    order = np.argsort(-res["logit"], axis=1)
    R = order.shape[0]
    if res["logit"].shape[1] < 2:
        return pre, np.full(R, np.inf)
    i0, i1 = order[:, 0], order[:, 1]
    r = np.arange(R)
    gap = (res["logit"][r, i0] - res["logit"][r, i1]) / (bnd["logit"][r, i0] + bnd["logit"][r, i1])
    return pre, gap


# ---------------------------------------------------------------------------- the kernels' walk in fp32 (numpy, their order)
def _tree(v):
    """the xor tree over the 64 lanes (last axis): offsets 32 .. 1, v += v[lane ^ o] in fp32; every lane ends the same"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(F)
    return v[..., 0]


def walk32(x, labels, w1, b1, w2, b2, lam, inv_rows):
    """both launches in fp32 in the kernels' order (expf / logf: numpy's float32 ones) -> dict keyed like rows64 + params64"""
    x, w1, b1, w2, b2 = (np.asarray(v, F) for v in (x, w1, b1, w2, b2))
    labels = np.asarray(labels, np.int64)
    R, D = x.shape
    H, S = w1.shape[0], w2.shape[0]
    lam, ir = F(lam), F(inv_rows)
    cnt = counted_rows(labels, S)
    acc = np.zeros((R, H), F)
    for dd in range(D):
        acc = fma(w1[None, :, dd], x[:, dd, None], acc)
    pre = (acc + b1).astype(F)
    h = np.where(pre > 0, pre, F(0)).astype(F)
    lanes = np.zeros((R, S, 64), F)
    npieces = H // 4
    for i in range(-(-npieces // 64)):
        pc = np.arange(64) + 64 * i
        ok = pc < npieces
        for k in range(4):
            j = np.where(ok, 4 * pc + k, 0)
            nxt = fma(w2[None, :, j], h[:, None, j], lanes)
            lanes = np.where(ok[None, None, :], nxt, lanes).astype(F)
    logit = (_tree(lanes) + b2).astype(F)
    m = logit.max(axis=1)
    pred = logit.argmax(axis=1)
    e = np.exp((logit - m[:, None]).astype(F)).astype(F)
    lanes = np.zeros((R, 64), F)
    for c0 in range(0, S, 64):
        blk = np.zeros((R, 64), F)
        blk[:, :min(64, S - c0)] = e[:, c0:c0 + 64]
        lanes = (lanes + blk).astype(F)
    s = _tree(lanes)
    inv = (F(1) / s).astype(F)
    lab = np.where(cnt, labels, 0)
    xl = (logit[np.arange(R), lab] - m).astype(F)
    loss = np.where(cnt, (np.log(s).astype(F) - xl).astype(F), F(0)).astype(F)
    onehot = np.zeros((R, S), F)
    onehot[np.nonzero(cnt)[0], labels[cnt]] = 1
    g2 = (ir * ((e * inv[:, None]).astype(F) - onehot).astype(F)).astype(F)
    g2 = np.where(cnt[:, None], g2, F(0)).astype(F)
    acc = np.zeros((R, H), F)
    for c in range(S):
        acc = fma(g2[:, c, None], w2[None, c, :], acc)
    g1 = np.where((h > 0) & cnt[:, None], acc, F(0)).astype(F)
    parts = []
    for q in range(NW):
        acc = np.zeros((R, D), F)
        for j in range(q * (H // NW), (q + 1) * (H // NW)):
            acc = fma(g1[:, j, None], w1[None, j, :], acc)
        parts.append(acc)
    tsum = parts[0]
    for q in range(1, NW):
        tsum = (tsum + parts[q]).astype(F)
    dx = (-(lam * tsum).astype(F)).astype(F)
    dx = np.where(cnt[:, None] & (lam != 0), dx, F(0)).astype(F)
    dw2, db2 = np.zeros((S, H), F), np.zeros(S, F)
    dw1, db1 = np.zeros((H, D), F), np.zeros(H, F)
    tot = 0.0
    for r in np.nonzero(cnt)[0]:
        dw2 = fma(g2[r, :, None], h[r, None, :], dw2)
        db2 = (db2 + g2[r]).astype(F)
        dw1 = fma(g1[r, :, None], x[r, None, :], dw1)
        db1 = (db1 + g1[r]).astype(F)
        tot += float(loss[r])
    hits = int((pred[cnt] == labels[cnt]).sum())
    out = np.array([F(tot), F(cnt.sum()), F(hits), F(tot * float(ir))], F)
    return dict(pre=pre, h=h, logit=logit, loss=loss, pred=pred, g2=g2, g1=g1, dx=dx, dw2=dw2, db2=db2, dw1=dw1, db1=db1,
                out=out)


# ------------------------------------------------------------------------------------------------------- seeded inputs
def make_case(name):
    """The seeded fp32 inputs of a GPU case: nn.Linear-like uniform weights, normal rows, labels from the generator; then
    every row whose smallest |pre| / bound or top-two logit gap / bound is below MARGIN is drawn again (from the same
    generator, a row at a time) until none is left: the GPU test then leaves no element out.  -> dict(x, labels, w1, b1, w2,
    b2, R, D, H, S, lam, inv_rows, ldx, col0)"""
    spec = CASES[name]
    R, D, H, S = spec["shape"]
    rng = np.random.default_rng(spec["seed"])
    k1, k2 = 1.0 / np.sqrt(D), 1.0 / np.sqrt(H)
    w1 = rng.uniform(-k1, k1, (H, D)).astype(F)
    b1 = rng.uniform(-k1, k1, H).astype(F)
    w2 = rng.uniform(-k2, k2, (S, H)).astype(F)
    b2 = rng.uniform(-k2, k2, S).astype(F)
    x = rng.standard_normal((R, D)).astype(F)
    labels = rng.integers(0, S, R).astype(np.int32)
    for r, v in spec.get("ignored", {}).items():
        labels[r] = v
    lam, inv_rows = float(F(0.5)), float(F(1.0 / R))
    for _ in range(200):
        res = rows64(x, labels, w1, b1, w2, b2, lam, inv_rows)
        pm, gm = margins(res, bounds(x, labels, w1, b1, w2, b2, lam, inv_rows, res))
        bad = np.nonzero((pm < MARGIN) | (gm < MARGIN))[0]
        if not bad.size:
            break
        x[bad] = rng.standard_normal((bad.size, D)).astype(F)
    else:
        raise RuntimeError(f"adv_ref.make_case({name}): rows {bad} stay within {MARGIN} bounds of a kink")
    return dict(x=x, labels=labels, w1=w1, b1=b1, w2=w2, b2=b2, R=R, D=D, H=H, S=S, lam=lam, inv_rows=inv_rows,
                ldx=D + spec.get("ldx_extra", 0) + spec.get("col0", 0), col0=spec.get("col0", 0))
