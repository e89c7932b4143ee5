"""The float64 restatement of the speaker adversary (tests/adv_ref.py) against torch autograd, its bounds against an fp32 walk in
the kernels' order and against three wrong kernels, the margins of the GPU cases' inputs, and the sign of the reversal.  CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import adv_ref as A
from ref_common import F, F64, worst_ratio

GRADS = ("dw1", "db1", "dw2", "db2")
ROWS = ("h", "loss", "g2", "g1", "dx")


@pytest.fixture(scope="module")
def cases():
    return {name: A.make_case(name) for name in A.CASES}


def both(c, lam=None):
    lam = c["lam"] if lam is None else lam
    args = (c["x"], c["labels"], c["w1"], c["b1"], c["w2"], c["b2"], lam, c["inv_rows"])
    res = A.rows64(*args)
    par = A.params64(c["x"], c["labels"], res, c["inv_rows"])
    return args, res, par


class Reverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lam):
        ctx.lam = lam
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return -ctx.lam * g, None


@pytest.mark.parametrize("name", ["one", "small", "odd", "step"])
def test_restatement_is_autograd_of_the_same_network(cases, name):
    c = cases[name]
    _, res, par = both(c)
    t = {k: torch.tensor(np.asarray(c[k], F64), requires_grad=True) for k in ("x", "w1", "b1", "w2", "b2")}
    labels = torch.tensor(c["labels"].astype(np.int64))
    keep = (labels >= 0) & (labels < c["S"])
    h = torch.relu(Reverse.apply(t["x"], c["lam"]) @ t["w1"].T + t["b1"])
    logits = h @ t["w2"].T + t["b2"]
    ce = Fn.cross_entropy(logits[keep], labels[keep], reduction="sum") * c["inv_rows"]
    ce.backward()
    close = lambda a, b: np.allclose(a, b, rtol=1e-11, atol=1e-14)
    assert close(par["out"][3], ce.item()) and close(par["out"][0] * c["inv_rows"], ce.item())
    assert close(res["dx"], t["x"].grad.numpy())
    for k, p in (("dw1", "w1"), ("db1", "b1"), ("dw2", "w2"), ("db2", "b2")):
        assert close(par[k], t[p].grad.numpy()), k
    assert par["out"][1] == int(keep.sum()) and par["out"][2] == int((logits.argmax(1)[keep] == labels[keep]).sum())
    assert np.array_equal(res["pred"], logits.argmax(1).numpy())
    # an ignored row: no loss, no gradient
    for r in np.nonzero(~res["counted"])[0]:
        assert res["loss"][r] == 0 and not res["g2"][r].any() and not res["g1"][r].any() and not res["dx"][r].any()


@pytest.mark.parametrize("name", list(A.CASES))
def test_fp32_walk_in_the_kernels_order_stays_inside_the_bounds(cases, name):
    c = cases[name]
    args, res, par = both(c)
    bnd = A.bounds(*args, res=res)
    w = A.walk32(*args)
    worst = {}
    for k in ROWS:
        worst[k], _ = worst_ratio(w[k], res[k], bnd[k])
    for k in GRADS:
        worst[k], _ = worst_ratio(w[k], par[k], bnd[k])
    worst["out"], _ = worst_ratio(w["out"][[0, 3]], par["out"][[0, 3]], bnd["out"][[0, 3]])
    print(name, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    assert np.array_equal(w["pred"], res["pred"]) and np.array_equal(w["out"][1:3], par["out"][1:3])


def test_bounds_are_not_vacuous(cases):
    """a flipped sign of dx, a dropped row and softmax without the one-hot each leave the bounds"""
    c = cases["step"]
    args, res, par = both(c)
    bnd = A.bounds(*args, res=res)
    assert worst_ratio(-res["dx"], res["dx"], bnd["dx"])[0] > 100
    last = np.nonzero(res["counted"])[0][-1]
    for k, wrong in (("dw2", par["dw2"] - np.outer(res["g2"][last], res["h"][last])), ("db2", par["db2"] - res["g2"][last]),
                     ("dw1", par["dw1"] - np.outer(res["g1"][last], c["x"][last])), ("db1", par["db1"] - res["g1"][last])):
        assert worst_ratio(wrong, par[k], bnd[k])[0] > 100, k
    assert worst_ratio(c["inv_rows"] * res["p"], res["g2"], bnd["g2"])[0] > 100
    # ... and they are small: a relative 1e-3 of the largest element is outside everywhere
    for k, ref in [(k, res[k]) for k in ROWS] + [(k, par[k]) for k in GRADS]:
        assert (bnd[k] <= 1e-3 * np.abs(ref).max()).all(), k


@pytest.mark.parametrize("name", list(A.CASES))
def test_gpu_cases_keep_their_distance_from_every_kink(cases, name):
    c = cases[name]
    args, res, _ = both(c)
    pm, gm = A.margins(res, A.bounds(*args, res=res))
    assert pm.min() >= A.MARGIN and gm.min() >= A.MARGIN, (pm.min(), gm.min())
    # both sides of the relu occur, and (beyond the one-row case) correct and wrong predictions do not matter: labels are random
    assert (res["pre"] > 0).any() and (res["pre"] < 0).any()
    spec = A.CASES[name]
    assert (~res["counted"]).sum() == len(spec.get("ignored", {}))
    if "ignored" in spec:
        lab = c["labels"][~res["counted"]]
        assert (lab < 0).any() and (lab >= c["S"]).any()


def test_descent_along_dx_raises_the_cross_entropy(cases):
    """the sign: dx is the gradient handed to q_mu, so the model's descent step x - eta dx must make the classifier WORSE"""
    c = cases["step"]
    args, res, par = both(c)
    assert np.abs(res["dx"]).max() > 0
    for eta in (1e-3, 1e-2):
        moved = A.rows64(c["x"].astype(F64) - eta * res["dx"], *args[1:])
        ce = A.params64(c["x"], c["labels"], moved, c["inv_rows"])["out"][3]
        assert ce > par["out"][3]
    # first order: the rise is eta |dx|^2 / lam
    rise = ce - par["out"][3]
    assert np.isclose(rise, 1e-2 * (res["dx"] ** 2).sum() / c["lam"], rtol=0.05)
    # lam = 0: exactly nothing reaches the model
    _, r0, _ = both(c, lam=0.0)
    assert not r0["dx"].any() and not np.signbit(r0["dx"]).any()
