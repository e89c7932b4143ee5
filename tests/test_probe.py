"""Speaker-identity probe (dvae_amd.probe) on the host: the float64 restatement of the fused softmax
cross-entropy kernel against torch's float64 cross_entropy, the chunk list and its by-utterance split, the padding helpers
and the CLI's refusal of a run without a checkpoint.  `softmax_ce_ref` is also the yardstick of tests/test_hip_probe.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dvae_amd  # noqa: E402,F401
from dvae_amd import probe as pr  # noqa: E402


# ----------------------------------------------------------------------------------------- float64 restatement
def softmax_ce_ref(logits, labels, classes, grad_scale=1.0):
    """dvae_softmax_ce in float64 numpy: logits [rows, ld], labels [rows] (negative: ignored) ->
    (row_loss [rows], row_pred [rows], dlogits [rows, ld] with zero padding columns, out [3] = loss sum, counted, correct)"""
    x = np.asarray(logits, dtype=np.float64)
    rows, ld = x.shape
    lab = np.asarray(labels).astype(np.int64).reshape(rows)
    z = x[:, :classes]
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    counted = lab >= 0
    safe = np.where(counted, lab, 0)
    at = np.arange(rows)
    row_loss = np.where(counted, np.log(s[:, 0]) - (z[at, safe] - m[:, 0]), 0.0)
    row_pred = z.argmax(1)                      # numpy returns the first (lowest) index of a tie
    onehot = np.zeros_like(z)
    onehot[at, safe] = 1.0
    d = np.zeros((rows, ld))
    d[:, :classes] = grad_scale * (e / s - onehot)
    d[~counted] = 0.0
    out = np.array([row_loss[counted].sum(), counted.sum(), (row_pred == lab)[counted].sum()], dtype=np.float64)
    return row_loss, row_pred, d, out


def top2_margin(logits, classes):
    """float64 gap between the largest and the second largest of each row's first `classes` logits (inf for one class)"""
    z = np.sort(np.asarray(logits, dtype=np.float64)[:, :classes], axis=1)
    return z[:, -1] - z[:, -2] if classes > 1 else np.full(z.shape[0], np.inf)


@pytest.mark.parametrize("rows,classes,ld", [(1, 1, 4), (7, 5, 8), (33, 109, 112), (9, 1000, 1000)])
def test_ref_is_torch_cross_entropy_in_float64(rows, classes, ld):
    rs = np.random.RandomState(rows + classes)
    x = rs.randn(rows, ld) * 3.0
    lab = rs.randint(0, classes, rows)
    lab[::3] = -1
    gs = 0.37
    row_loss, row_pred, d, out = softmax_ce_ref(x, lab, classes, gs)
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tl = torch.nn.functional.cross_entropy(t[:, :classes], torch.tensor(lab), ignore_index=-1, reduction="none")
    (gs * tl.sum()).backward()
    assert np.max(np.abs(row_loss - tl.detach().numpy())) <= 1e-12
    assert np.max(np.abs(d - t.grad.numpy())) <= 1e-12
    assert np.all(d[:, classes:] == 0.0) and np.all(d[lab < 0] == 0.0) and np.all(row_loss[lab < 0] == 0.0)
    assert np.array_equal(row_pred, t[:, :classes].argmax(1).numpy())
    assert abs(out[0] - float(tl.sum())) <= 1e-12 * max(1.0, abs(out[0]))
    assert out[1] == (lab >= 0).sum() and out[2] == (row_pred == lab).sum()
    if (lab >= 0).any():      # the mean the autograd function returns
        tm = torch.nn.functional.cross_entropy(t[:, :classes], torch.tensor(lab), ignore_index=-1)
        assert abs(out[0] / out[1] - float(tm)) <= 1e-12


def test_ref_ties_and_offset():
    x = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]]) + 1e4
    row_loss, row_pred, d, _ = softmax_ce_ref(x, [2, 0], 3)
    assert row_pred.tolist() == [1, 0]
    assert np.all(np.isfinite(row_loss)) and np.all(np.isfinite(d))
    assert abs(row_loss[1] - np.log(3.0)) <= 1e-12 and np.all(d[:, 3] == 0.0)


# ------------------------------------------------------------------------------------------------------ chunk list
LENGTHS = (63, 64, 65, 128, 200, 130)


def write_corpus(root, lengths=LENGTHS, n_speakers=3):
    rs = np.random.RandomState(0)
    for s in range(n_speakers):
        d = os.path.join(root, f"spk{s}")
        os.makedirs(d)
        for u, n in enumerate(lengths):
            np.save(os.path.join(d, f"utt{u:02d}_mel.npy"), rs.uniform(0, 1, (80, n)).astype(np.float32))
    return root


def test_list_chunks_counts_and_split(tmp_path):
    ch = pr.list_chunks(write_corpus(str(tmp_path / "c")), 64)
    assert ch.speakers == ["spk0", "spk1", "spk2"]
    assert len(ch.skipped) == 3 and all(p.endswith("utt00_mel.npy") for p in ch.skipped)
    for s in range(3):
        us = [u for u in ch.utterances if u["speaker"] == s]
        assert [u["position"] for u in us] == [1, 2, 3, 4, 5]
        assert [u["n_chunks"] for u in us] == [1, 1, 2, 3, 2]
        assert [u["held_out"] for u in us] == [False, False, False, True, False]     # exactly the one at position 4
    assert len(ch) == 3 * 9 and int(ch.held_out.sum()) == 3 * 3
    # the per-chunk arrays say the same, no chunk reads past its utterance, and no utterance is on both sides
    for k in range(len(ch)):
        u = ch.utterances[ch.utt[k]]
        assert ch.held_out[k] == u["held_out"] and ch.speaker[k] == u["speaker"]
        assert ch.start[k] % 64 == 0 and ch.start[k] + 64 <= u["length"]
    train_utts, held_utts = set(ch.utt[~ch.held_out].tolist()), set(ch.utt[ch.held_out].tolist())
    assert train_utts and held_utts and not (train_utts & held_utts)
    assert ch.speaker.dtype == np.int32


def test_list_chunks_max_utts_and_too_few(tmp_path):
    root = write_corpus(str(tmp_path / "c"), lengths=(64,) * 12)
    ch = pr.list_chunks(root, 64, max_utts=10)
    assert len(ch.utterances) == 30 and sorted({u["position"] for u in ch.utterances if u["held_out"]}) == [4, 9]
    # 4 usable utterances (the fifth is too short): an error that names the speaker
    bad = write_corpus(str(tmp_path / "d"), lengths=(64, 64, 64, 64, 10), n_speakers=2)
    with pytest.raises(ValueError, match="spk0"):
        pr.list_chunks(bad, 64)


def test_padding_helpers():
    assert pr.pad_width(4) == 4 and pr.pad_width(28) == 28 and pr.pad_width(109) == 112 and pr.pad_width(5) == 8
    assert pr.pad_width(1) == 4 and pr.pad_width(1000) == 1000


def test_cli_without_checkpoint_exits_nonzero(tmp_path):
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.json").write_text(json.dumps(dict(samples_length=64, latent_size=32, speaker_size=4)))
    write_corpus(str(tmp_path / "c"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "dvae_amd.probe", str(tmp_path / "c"), "--log_dir", str(run)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0, r.stdout
    assert "no checkpoint under" in r.stderr and "train the model first" in r.stderr, r.stderr
    assert not (run / "probe.json").exists()
