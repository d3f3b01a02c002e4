"""Train splits for the negative-sampling tests (tests/test_negative_sample_*.py), from lime_cikm25_amd.synth's counter-based generator:
records in the 11-field layout of ``Corpus.train_behaviors`` (corpus.py:539-552) with a chosen number of non-clicked news each."""
import numpy as np

from lime_cikm25_amd import synth


def records(counts, H=6, n_news=500, seed=0):
    """One train record per entry of ``counts`` with that many non-clicked news.  The non-clicked news of a record are DISTINCT news
    indices and their lifetimes distinct values, so a drawn news index identifies the position it was drawn from."""
    counts = np.asarray(counts, dtype=np.int64)
    N, nnz = counts.size, int(counts.sum())
    assert counts.max() < n_news - 1
    start = synth.randint('neg.start', seed, N, 0, n_news - 1)
    step = np.arange(nnz) - np.repeat(np.cumsum(counts) - counts, counts)
    neg = (1 + (np.repeat(start, counts) + step) % (n_news - 1)).astype(np.int64)          # a run of consecutive indices in [1, n_news)
    neg_lt = (600.0 + step * 7.0 + np.repeat(synth.uniform01('neg.lt', seed, N), counts)).astype(np.float32).astype(np.float64)
    pos = synth.randint('neg.pos', seed, N, 1, n_news)
    uid = synth.randint('neg.uid', seed, N, 0, 50)
    fresh = np.exp(np.log(60.0) + synth.uniform01('neg.cfr', seed, N) * np.log(43200.0)).astype(np.float32).astype(np.float64)
    pos_lt = np.exp(np.log(600.0) + synth.uniform01('neg.plt', seed, N) * np.log(2016.0)).astype(np.float32).astype(np.float64)
    n_hist = synth.randint('neg.hn', seed, N, 0, H + 1)
    hist = synth.randint('neg.h', seed, N * H, 1, n_news).reshape(N, H)
    mask = np.arange(H)[None, :] < n_hist[:, None]
    hist = np.where(mask, hist, 0).astype(np.int32)
    n_list = synth.randint('neg.ln', seed, N, 0, H + 4)                                     # shorter and longer than H
    ufr = synth.uniform01('neg.ufr', seed, N * (H + 4)).reshape(N, H + 4) * 86400.0
    ult = synth.uniform01('neg.ult', seed, N * (H + 4)).reshape(N, H + 4) * 86400.0
    neg_l, lt_l, o = neg.tolist(), neg_lt.tolist(), (np.cumsum(counts) - counts).tolist()
    out = []
    for i, (c, s) in enumerate(zip(counts.tolist(), o)):
        out.append([int(uid[i]), hist[i], mask[i], int(pos[i]), neg_l[s:s + c], i, float(fresh[i]), float(pos_lt[i]), lt_l[s:s + c],
                    ufr[i, :n_list[i]].tolist(), ult[i, :n_list[i]].tolist()])
    return out


def split(cfg, counts, seed=0):
    """A ``synth.synth_corpus`` whose train records are ``records(counts)`` (news indices inside its news tables)."""
    corpus = synth.synth_corpus(cfg, n_news=500, n_train=1, n_dev=2, seed=seed)
    corpus.train_behaviors = records(counts, H=cfg.max_history_num, n_news=500, seed=seed)
    return corpus


def mixed_counts(N, seed=0, lo=1, hi=71):
    """``N`` counts, uniform over lo .. hi."""
    return synth.randint('neg.count', seed, N, lo, hi + 1)


def tables(samples, freshness, lifetime):
    """The three lists of negative_sampling / counter_negative_sampling as the arrays DeviceBehaviors uploads."""
    return np.asarray(samples, dtype=np.int32), np.asarray(freshness, dtype=np.float32), np.asarray(lifetime, dtype=np.float32)

