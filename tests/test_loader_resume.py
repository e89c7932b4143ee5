"""data.GpuPairLoader.skip_epochs on the CPU (no adversary, no device work: `gather` is replaced): a loader that skipped e epochs
feeds, in epoch e + 1, the batches — utterances, crop offsets, speakers — that a loader which iterated e epochs feeds, and one
without a seed has nothing to replay."""
import numpy as np
import pytest

from dvae_amd.data import GpuPairLoader, SpeechDatasetGVAE, write_synthetic_corpus


class HostLoader(GpuPairLoader):
    def gather(self, utt, off):
        return tuple(int(v) for v in utt), tuple(int(v) for v in off)


def make(corpus, seed=3, **kw):
    return HostLoader(SpeechDatasetGVAE(corpus, samples_length=64, seed=seed), 4, device="cpu", seed=seed, **kw)


def epoch(loader):
    out = [(a, b, tuple(s.tolist())) for a, b, s in loader]
    loader.dataset.shuffle_data()          # what train() does at the end of an epoch
    return out


@pytest.mark.parametrize("skipped", [1, 3])
@pytest.mark.parametrize("world", [1, 2])
def test_skipped_epochs_are_the_iterated_ones(tmp_path, skipped, world):
    corpus = write_synthetic_corpus(str(tmp_path / "c"), n_speakers=2, n_utt=16, length=96, seed=0)
    kw = dict(rank=world - 1, world_size=world)
    a = make(corpus, **kw)
    seen = [epoch(a) for _ in range(skipped + 1)]
    b = make(corpus, **kw)
    b.skip_epochs(skipped)
    assert epoch(b) == seen[skipped]
    assert seen[skipped] != seen[0] and len(seen[0]) == 4 // world
    assert any(o for batch in seen[0] for o in batch[0][1]), "the crops are random: the offsets are part of what is replayed"
    c = make(corpus, **kw)
    c.skip_epochs(0)
    assert epoch(c) == seen[0]


def test_without_a_seed_there_is_nothing_to_replay(tmp_path):
    corpus = write_synthetic_corpus(str(tmp_path / "c"), n_speakers=2, n_utt=8, length=96, seed=0)
    loader = HostLoader(SpeechDatasetGVAE(corpus, samples_length=64, seed=1), 4, device="cpu", seed=None)
    state = np.random.get_state()[1].copy()
    pairs = loader.dataset.utterance_fp.copy()
    loader.skip_epochs(2)
    assert np.array_equal(np.random.get_state()[1], state) and np.array_equal(loader.dataset.utterance_fp, pairs)
