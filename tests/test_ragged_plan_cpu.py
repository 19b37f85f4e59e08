"""The offline planner's batches of similar-length rows (rvcx/offline.py bucket, plan(max_pad=)); no GPU."""
import numpy as np
import pytest

from rvcx import offline
from rvcx.engine import hubert_frames


def mixed_job(n_utt=97, seed=7):
    """Lengths of 0.5-30 s, with a few repeated so equal-length groups exist too."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ns = rng.integers(8000, 480000, size=n_utt).tolist()
    ns[10:20] = [160000] * 10
    ns[40:43] = [32000] * 3
    return [offline.Utterance(i, int(n), 1000 + i) for i, n in enumerate(ns)]


@pytest.mark.parametrize("batch", [1, 4, 8, 16])
@pytest.mark.parametrize("max_pad", [0.0, 0.05, 0.125, 0.25, 0.9])
def test_bucket_invariants(batch, max_pad):
    ns = [u.n for u in mixed_job()]
    groups = offline.bucket(ns, batch, max_pad)
    assert sorted(i for g in groups for i in g) == list(range(len(ns)))  # every row exactly once
    for g in groups:
        assert 1 <= len(g) <= batch
        lens = [ns[i] for i in g]
        assert min(lens) >= (1.0 - max_pad) * max(lens)
        assert lens == sorted(lens, reverse=True)  # the longest row comes first
    # greedy over the sorted rows: a batch is closed only when it is full or the next row would break the rule
    for g, h in zip(groups, groups[1:]):
        assert len(g) == batch or ns[h[0]] < (1.0 - max_pad) * ns[g[0]]


def test_bucket_rejects_bad_arguments():
    with pytest.raises(ValueError):
        offline.bucket([1, 2], 0, 0.1)
    with pytest.raises(ValueError):
        offline.bucket([1, 2], 2, 1.0)
    with pytest.raises(ValueError):
        offline.bucket([1, 2], 2, -0.1)
    assert offline.bucket([], 4, 0.1) == []


def _today(job, world, rank, batch):
    """plan() as it was before max_pad existed, written out: LPT shard, equal lengths, longest first."""
    shard = offline.assign_lpt([u.n for u in job], world)[rank]
    by_len = {}
    for i in shard:
        by_len.setdefault(job[i].n, []).append(i)
    batches = []
    for n in sorted(by_len, reverse=True):
        batches += [by_len[n][k:k + batch] for k in range(0, len(by_len[n]), batch)]
    return shard, batches


@pytest.mark.parametrize("job", [offline.c4_job(), mixed_job()], ids=["c4", "mixed"])
@pytest.mark.parametrize("world,batch", [(1, 4), (8, 4), (3, 16)])
def test_max_pad_none_is_todays_plan(job, world, batch):
    for rank in range(world):
        p = offline.plan(job, world, rank, batch)
        q = offline.plan(job, world, rank, batch, max_pad=None)
        shard, batches = _today(job, world, rank, batch)
        assert p.shard == q.shard == shard and p.batches == q.batches == batches


@pytest.mark.parametrize("job", [offline.c4_job(64), mixed_job()], ids=["c4", "mixed"])
def test_max_pad_zero_is_equal_length_grouping(job):
    for rank in range(3):
        assert offline.plan(job, 3, rank, 4, max_pad=0.0).batches == offline.plan(job, 3, rank, 4).batches


def test_shards_do_not_depend_on_max_pad():
    job = mixed_job()
    for rank in range(8):
        base = offline.plan(job, 8, rank, 8)
        for mp in (0.0, 0.05, 0.25):
            p = offline.plan(job, 8, rank, 8, max_pad=mp)
            assert p.shard == base.shard
            assert sorted(i for b in p.batches for i in b) == sorted(base.shard)
            for b in p.batches:
                lens = [job[i].n for i in b]
                assert len(b) <= 8 and min(lens) >= (1.0 - mp) * max(lens)


def test_hubert_frames_counts_the_feature_encoder():
    """The frame counts the ragged HuBERT test relies on, and the first length that gives a frame."""
    assert [hubert_frames(n) for n in (40000, 400, 21000, 20700, 16000)] == [124, 1, 65, 64, 49]
    assert hubert_frames(399) == 0 and hubert_frames(0) == 0
    assert all(hubert_frames(n) == (n - 400) // 320 + 1 for n in np.arange(400, 4000, 37).tolist())
