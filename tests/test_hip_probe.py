"""Speaker-identity probe on the MI355X (dvae_amd.probe, csrc/probe.hip): the fused softmax cross-entropy
kernel against the float64 restatement of tests/test_probe.py, the autograd function's gradients through the classifier
against float64 torch.autograd, the classifier on planted data, and the CLI end to end.

Tolerances of the kernel (derived, not tuned): an fp32 evaluation in numpy differs from float64 by at most
1.3e-7 * max(1, max|x|) in a row's loss and 2.9e-7 in a probability (measured on the CPU for 5, 109 and 1000 classes, scales
3, 10 and 30 and the +1e4 offset); the device is allowed 2e-6 * max(1, max|logits_row|) per row loss and 4e-6 * grad_scale
per gradient element — about 15 x that, for an exp / log a few ulp looser.  A real fault (a missed column, a padding
column read, no maximum subtracted) is off by at least 1e-3 on these inputs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_amd  # noqa: E402,F401
from dvae_amd import ops, probe as pr  # noqa: E402
from dvae_amd._lib import lib, ptr, stream  # noqa: E402
from test_mcd import harmonic, write_pcm16  # noqa: E402
from test_probe import softmax_ce_ref, top2_margin  # noqa: E402

SHAPES = [(1, 1, 4), (3, 2, 4), (5, 5, 8), (257, 64, 64), (257, 65, 68), (130, 109, 112), (66, 1000, 1000),
          (33, 1024, 1024)]
LOSS_TOL, GRAD_TOL, MARGIN = 2e-6, 4e-6, 1e-5


def make(rows, classes, ld, kind="normal", seed=0):
    rs = np.random.RandomState(1000 * seed + rows + 7 * classes)
    x = (rs.randn(rows, ld) * 3.0).astype(np.float32)
    lab = rs.randint(0, classes, rows).astype(np.int32)
    if kind == "offset":
        x = (x + np.float32(1e4)).astype(np.float32)
    elif kind == "ties":
        x = rs.randint(-2, 3, (rows, ld)).astype(np.float32)      # many exact ties of the maximum
    elif kind == "ignored":
        lab[::3] = -1
    x[:, classes:] = 1e30       # a padding column that is read, or not overwritten, shows
    return x, lab


def run(x, lab, classes, gs=1.0, grad=True, inplace=False):
    """-> (row_loss, row_pred, dlogits or None, out[4]) as numpy, through ops.softmax_ce"""
    xd = torch.from_numpy(x).cuda()
    ld = torch.from_numpy(lab).cuda()
    d = None
    if grad:
        d = xd if inplace else torch.full_like(xd, float("nan"))
    row_loss, row_pred, out = ops.softmax_ce(xd, ld, classes, gs, d)
    torch.cuda.synchronize()
    return (row_loss.cpu().numpy(), row_pred.cpu().numpy(), None if d is None else d.cpu().numpy(), out.cpu().numpy())


def check_against_ref(x, lab, classes, gs, got):
    row_loss, row_pred, d, out = got
    r_loss, r_pred, r_d, r_out = softmax_ce_ref(x, lab, classes, gs)
    rows = x.shape[0]
    bound = LOSS_TOL * np.maximum(1.0, np.abs(x[:, :classes].astype(np.float64)).max(1))
    err = np.abs(row_loss - r_loss)
    print(f"rows {rows} classes {classes} ld {x.shape[1]}: loss err {err.max():.3e} (bound {bound.min():.3e}), "
          f"grad err {np.abs(d - r_d).max() / gs:.3e} (bound {GRAD_TOL:.1e}), out {out[:3]} ref {r_out}")
    assert np.all(np.isfinite(row_loss)) and np.all(np.isfinite(d))
    assert np.all(err <= bound), (err.max(), bound.min())
    assert np.max(np.abs(d - r_d)) <= GRAD_TOL * gs
    sure = top2_margin(x, classes) > MARGIN
    assert np.array_equal(row_pred[sure], r_pred[sure])
    assert np.all((row_pred >= 0) & (row_pred < classes))
    assert np.all(d[:, classes:] == 0.0)
    assert np.all(d[lab < 0] == 0.0) and np.all(row_loss[lab < 0] == 0.0)
    assert abs(out[0] - r_out[0]) <= rows * bound.max()
    assert out[1] == r_out[1]
    assert out[2] == ((row_pred == lab) & (lab >= 0)).sum()
    if np.all(sure):
        assert out[2] == r_out[2]
    if r_out[1] > 0:
        assert abs(out[3] - r_out[0] / r_out[1]) <= bound.max()


# ------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("kind", ["normal", "offset", "ignored"])
@pytest.mark.parametrize("rows,classes,ld", SHAPES)
def test_softmax_ce_against_float64(rows, classes, ld, kind):
    x, lab = make(rows, classes, ld, kind)
    gs = 1.0 / rows if kind != "offset" else 0.5
    check_against_ref(x, lab, classes, gs, run(x, lab, classes, gs))


@pytest.mark.parametrize("rows,classes,ld", [(5, 5, 8), (257, 65, 68), (33, 1024, 1024)])
def test_ties_take_the_lowest_index(rows, classes, ld):
    x, lab = make(rows, classes, ld, "ties")
    got = run(x, lab, classes, 1.0)
    assert np.array_equal(got[1], softmax_ce_ref(x, lab, classes)[1])       # every row: the margins are 0 or >= 1
    assert (top2_margin(x, classes) == 0).sum() >= rows // 2
    check_against_ref(x, lab, classes, 1.0, got)


def test_evaluation_without_gradient_and_in_place():
    rows, classes, ld = 257, 65, 68
    x, lab = make(rows, classes, ld, "ignored")
    ref = run(x, lab, classes, 0.25)
    ev = run(x, lab, classes, 0.25, grad=False)
    assert ev[2] is None
    for a, b in ((ref[0], ev[0]), (ref[1], ev[1]), (ref[3], ev[3])):
        assert np.array_equal(a, b)
    ip = run(x.copy(), lab, classes, 0.25, inplace=True)
    for a, b in zip(ref, ip):
        assert np.array_equal(a, b)
    e3 = ops.softmax_ce_eval(torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), classes).cpu().numpy()
    assert np.array_equal(e3, ref[3][:3])


def test_batch_independence_and_determinism():
    rows, classes, ld = 257, 65, 68
    x, lab = make(rows, classes, ld)
    full = run(x, lab, classes, 1.0 / rows)
    again = run(x, lab, classes, 1.0 / rows)
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    alone = run(x[:10].copy(), lab[:10].copy(), classes, 1.0 / rows)
    for a, b in zip(full[:3], alone[:3]):
        assert np.array_equal(a[:10], b)


@pytest.mark.parametrize("rows,classes,ld", [(4, 0, 4), (4, 1025, 1028), (4, 6, 4), (4, 5, 6), (0, 5, 8)])
def test_bad_arguments_are_refused(rows, classes, ld):
    n = 8 * 1028
    x = torch.zeros(n, device="cuda")
    lab = torch.zeros(8, device="cuda", dtype=torch.int32)
    d = torch.full((n,), 7.0, device="cuda")
    row_loss = torch.full((8,), 7.0, device="cuda")
    row_pred = torch.full((8,), 7, device="cuda", dtype=torch.int32)
    out = torch.full((4,), 7.0, device="cuda")
    rc = lib().dvae_softmax_ce(ptr(x), ptr(lab), ptr(d), ptr(row_loss), ptr(row_pred), ptr(out), rows, classes, ld, 1.0,
                               stream())
    torch.cuda.synchronize()
    assert rc == -1
    for t in (d, row_loss, out):
        assert bool((t == 7.0).all())
    assert bool((row_pred == 7).all())
    with pytest.raises(Exception):
        ops.softmax_ce(x[:32].view(4, 8), lab[:4], 9)


# --------------------------------------------------------------------------------------------------- autograd function
def test_softmax_ce_fn_gradients_through_the_probe():
    dim, hidden, classes, rows = 4, 1024, 5, 130
    p = pr.SpeakerProbe(dim, classes, hidden=hidden, seed=3)
    assert (p.dim_p, p.classes_p) == (4, 8)
    rs = np.random.RandomState(5)
    x = rs.randn(rows, dim).astype(np.float32)
    y = rs.randint(0, classes, rows).astype(np.int32)
    xs = torch.from_numpy(x).cuda()
    p.optimizer.zero_grad()
    loss = p.loss(xs, torch.from_numpy(y).cuda(), rows)
    loss.backward()
    torch.cuda.synchronize()
    flat_g = p.optimizer.flat_g.cpu().numpy().astype(np.float64)
    # float64 torch.autograd on the same (padded) parameters
    ref = {k: v.detach().cpu().double().requires_grad_(True) for k, v in p.params.items()}
    h = torch.relu(torch.from_numpy(x).double() @ ref["w1"].T + ref["b1"])
    lg = h @ ref["w2"].T + ref["b2"]
    rl = torch.nn.functional.cross_entropy(lg[:, :classes], torch.from_numpy(y).long())
    rl.backward()
    assert abs(float(loss) - float(rl)) <= 1e-4 * abs(float(rl))
    for name, par in p.params.items():
        o = p.optimizer.offsets[name]
        got = flat_g[o:o + par.numel()].reshape(tuple(par.shape))
        want = ref[name].grad.numpy()
        scale = np.abs(want).max()
        print(f"{name}: max err {np.abs(got - want).max():.3e} of max abs {scale:.3e}")
        assert np.abs(got - want).max() <= 1e-4 * scale, name
    o2, ob = p.optimizer.offsets["w2"], p.optimizer.offsets["b2"]
    gw2 = flat_g[o2:o2 + 8 * hidden].reshape(8, hidden)
    assert np.all(gw2[classes:] == 0.0) and np.all(flat_g[ob + classes:ob + 8] == 0.0)
    # a feature width that needs padding: the padding columns of the first layer's gradient are exactly zero too
    q = pr.SpeakerProbe(6, classes, hidden=64, seed=1)
    xq = q.standardise(rs.randn(rows, 6).astype(np.float32))
    q.optimizer.zero_grad()
    q.loss(xq, torch.from_numpy(y).cuda(), rows).backward()
    torch.cuda.synchronize()
    o1 = q.optimizer.offsets["w1"]
    gw1 = q.optimizer.flat_g[o1:o1 + 64 * 8].view(64, 8).cpu().numpy()
    assert np.all(gw1[:, 6:] == 0.0) and np.abs(gw1[:, :6]).max() > 0


# ------------------------------------------------------------------------------------------------------ planted data
def planted(sep, seed=11, classes=5, dim=4, n_train=2000, n_held=1000):
    rs = np.random.RandomState(seed)
    centres = rs.randn(classes, dim) * sep
    y = rs.randint(0, classes, n_train + n_held).astype(np.int32)
    x = (centres[y] + rs.randn(n_train + n_held, dim)).astype(np.float32)
    return x[:n_train], y[:n_train], x[n_train:], y[n_train:]


@pytest.fixture(scope="module")
def fitted():
    out = {}
    for sep in (4, 0):
        xt, yt, xh, yh = planted(sep)
        p = pr.SpeakerProbe(4, 5, seed=0)
        losses = p.fit(torch.from_numpy(xt).cuda(), yt, epochs=20, batch=512)
        out[sep] = (p, list(losses), p.evaluate(xt, yt), p.evaluate(xh, yh))
    return out


def test_fit_separates_planted_classes(fitted):
    p, losses, tr, ho = fitted[4]
    print("sep 4:", tr, ho, losses[0], losses[-1])
    assert len(losses) == 20 and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert ho["n"] == 1000 and tr["n"] == 2000
    assert ho["accuracy"] >= 0.98
    hit = (p.predict(planted(4)[2]).cpu().numpy() == planted(4)[3]).mean()
    assert abs(hit - ho["accuracy"]) < 1e-12
    lp = p.log_prob(planted(4)[2]).cpu().numpy().astype(np.float64)
    assert lp.shape == (1000, 5) and np.max(np.abs(np.exp(lp).sum(1) - 1.0)) <= 1e-5
    assert np.mean(lp.argmax(1) == planted(4)[3]) >= 0.98


def test_fit_finds_nothing_without_structure(fitted):
    _, losses, tr, ho = fitted[0]
    print("sep 0:", tr, ho, losses[0], losses[-1])
    assert np.all(np.isfinite(losses))
    assert ho["accuracy"] <= 0.25                     # chance 0.2 + 4 sigma of a binomial with n = 1000
    assert tr["accuracy"] > ho["accuracy"] - 0.05     # something was fitted


def test_fit_is_bit_reproducible(fitted):
    xt, yt, _, _ = planted(4)
    p = pr.SpeakerProbe(4, 5, seed=0)
    p.fit(torch.from_numpy(xt).cuda(), yt, epochs=20, batch=512)
    assert torch.equal(p.optimizer.flat_p, fitted[4][0].optimizer.flat_p)
    # the short last minibatch (2000 = 3 * 512 + 464) was part of every epoch
    assert 2000 % 512 != 0


# ------------------------------------------------------------------------------------------------------- end to end
def _cli(args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "dvae_amd.probe"] + [str(a) for a in args], cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


LINE = re.compile(r"^probe (style|content): held-out accuracy ([0-9.]+) \(train ([0-9.]+), chance ([0-9.]+), (\d+) held-out "
                  r"chunks of (\d+) utterances, (\d+) speakers\)$")


def test_cli_end_to_end(tmp_path):
    from dvae_amd.data import write_synthetic_corpus
    corpus = write_synthetic_corpus(str(tmp_path / "corpus"), n_speakers=3, n_utt=10, length=130)
    run_dir = tmp_path / "run"
    (run_dir / "checkpoints").mkdir(parents=True)
    cfg = dict(samples_length=64, latent_size=32, speaker_size=4, lr=1e-4, batch_size=4, mse_cof=10, kl_cof=10)
    (run_dir / "config.json").write_text(json.dumps(cfg))
    torch.manual_seed(0)
    vsc = dvae_amd.ConvolutionalMulVAE("VCTK", 64, 80, 32, 1e-4, 0.01, 500, False, batch_size=4, speaker_size=4,
                                       device=torch.device("cuda"), latent_dim=32)
    torch.save(vsc.model.state_dict(), run_dir / "checkpoints" / "DisentangledVAE_VCTK_3.pth")
    del vsc
    wavs = tmp_path / "wavs"
    wavs.mkdir()
    n = int(1.1 * 16000)
    write_pcm16(wavs / "convert_a_to_b_001.wav", harmonic(n, 120.0, seed=1))
    write_pcm16(wavs / "convert_a_to_b_002.wav", harmonic(n, 210.0, seed=2))
    args = [corpus, "--log_dir", run_dir, "--epochs", 3, "--seed", 1, "--score", wavs, "--speaker", "spk001"]
    r = _cli(args)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    probes = [LINE.match(ln) for ln in lines if ln.startswith("probe ")]
    assert len(probes) == 2 and all(probes), lines
    assert [m.group(1) for m in probes] == ["style", "content"]
    for m in probes:
        assert 0.0 <= float(m.group(2)) <= 1.0 and 0.0 <= float(m.group(3)) <= 1.0
        assert abs(float(m.group(4)) - 1 / 3) < 1e-3 and (int(m.group(5)), int(m.group(6)), int(m.group(7))) == (12, 6, 3)
    files = [ln for ln in lines if ln.startswith("file ")]
    assert len(files) == 2 and all(re.match(r"^file convert_a_to_b_00[12]\.wav: spk00[012]$", ln) for ln in files), lines
    assert re.match(r"^target speaker accuracy: [012]/2$", lines[-1]), lines
    res = json.loads((run_dir / "probe.json").read_text())
    assert res["speakers"] == ["spk000", "spk001", "spk002"] and res["checkpoint_epoch"] == 3 and res["skipped"] == []
    assert res["n_train_chunks"] == 48 and res["n_held_out_chunks"] == 12
    assert res["n_train_utterances"] == 24 and res["n_held_out_utterances"] == 6
    for name, dim in (("style", 4), ("content", 28)):
        pb = res["probes"][name]
        assert pb["dim"] == dim and pb["n_train_chunks"] == 48 and pb["n_held_out_chunks"] == 12 and pb["n_speakers"] == 3
        assert 0.0 <= pb["held_out_accuracy"] <= 1.0 and 0.0 <= pb["train_accuracy"] <= 1.0
        assert abs(pb["chance"] - 1 / 3) < 1e-12 and len(pb["epoch_losses"]) == 3
        assert sorted(pb["per_speaker_held_out_accuracy"]) == res["speakers"]
        assert all(0.0 <= v <= 1.0 for v in pb["per_speaker_held_out_accuracy"].values())
    for spk in res["speakers"]:
        st = res["style_stats"][spk]
        assert st["n_chunks"] == 20 and len(st["mean"]) == 4 and len(st["std"]) == 4 and min(st["std"]) >= 0.0
    sc = res["score"]
    assert sc["n"] == 2 and 0 <= sc["correct"] <= 2 and sc["speaker"] == "spk001"
    assert [f["file"] for f in sc["files"]] == ["convert_a_to_b_001.wav", "convert_a_to_b_002.wav"]
    assert all(f["n_chunks"] == 1 and f["predicted"] in res["speakers"] for f in sc["files"])
    # a second run writes the same file: encoder, fit and scoring are bit-reproducible
    r2 = _cli(args + ["--json", tmp_path / "second.json"])
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert (tmp_path / "second.json").read_text() == (run_dir / "probe.json").read_text()
    assert r2.stdout == r.stdout
