"""The counter-based negative sampling rule without a GPU: device_data.counter_negative_sampling / counter_negative_draws (the host
twin of lime_negative_sample, csrc/negative_sample.hip) against the reference's rule as device_data.negative_sampling states it
(dataset.py:42-77) -- equal where the rule is deterministic, the same support and the same distribution where it draws -- its
purity in (seed, epoch, record), and the argument checks of the C entry point, which need no device."""
import ctypes

import numpy as np
import pytest

import negative_sample_cases as cases
from lime_cikm25_amd import _lib, make_config, synth
from lime_cikm25_amd.build import build_library
from lime_cikm25_amd.device_data import counter_negative_draws, counter_negative_sampling, negative_sampling

K = 4
CHI2_10DF_999 = 29.59            # 0.999 quantile of chi-square with 10 degrees of freedom
CHI2_3DF_999 = 16.27             # ... with 3


def small_cfg(**kw):
    return make_config(max_history_num=6, max_title_length=8, max_abstract_length=16, batch_size=4, vocabulary_size=3000,
                       negative_sample_num=K, **kw)


def check_rows(beh, out, k, inclusive):
    """Every row against its record: positive first, freshness repeated, lifetimes of the drawn news, and for n > k distinct draws
    inside the support.  Returns the drawn positions of the n > k rows as (n, positions) pairs."""
    samples, freshness, lifetime = out
    assert len(samples) == len(freshness) == len(lifetime) == len(beh)
    drawn = []
    for rec, s, f, l in zip(beh, samples, freshness, lifetime):
        neg, n = rec[4], len(rec[4])
        assert len(s) == len(f) == len(l) == 1 + k
        assert s[0] == rec[3] and l[0] == rec[7] and f == [rec[6]] * (1 + k)
        where = [neg.index(x) for x in s[1:]]                      # cases.records: the non-clicked news of a record are distinct
        assert l[1:] == [rec[8][w] for w in where]
        if n <= k:
            assert where == [j % n for j in range(k)]
        else:
            assert len(set(where)) == k and min(where) >= 0 and max(where) <= (n - 1 if inclusive else n - 2), (n, where)
            drawn.append((n, where))
    return drawn


def test_equals_the_reference_rule_where_it_is_deterministic():
    cfg = small_cfg()
    corpus = synth.synth_corpus(cfg, n_train=40, n_neg_max=K)
    assert max(len(b[4]) for b in corpus.train_behaviors) == K
    want = negative_sampling(corpus.train_behaviors, K)
    for seed, epoch, inclusive in ((0, 1, False), (7, 3, True)):
        assert counter_negative_sampling(corpus.train_behaviors, K, seed, epoch, inclusive) == want


@pytest.mark.parametrize('k', [1, 4, 8])
def test_rows_are_well_formed_and_draws_stay_inside_the_support(k):
    cfg = small_cfg()
    toy = synth.synth_corpus(cfg, n_train=40, n_neg_max=9).train_behaviors
    for rec in toy:                                                # synth_corpus may repeat a news inside a record: make them distinct
        rec[4] = list(range(1, 1 + len(rec[4])))
    hand = cases.records([1, 2, 3, 4, 5, 6, 9, 10, 17, 33, 64, 65, 100, 299, 300, 300, 5, 5, 5, 6, 6, 6] * 6)
    for beh in (toy, hand):
        excl = check_rows(beh, counter_negative_sampling(beh, k, 11, 2), k, inclusive=False)
        incl = check_rows(beh, counter_negative_sampling(beh, k, 11, 2, inclusive=True), k, inclusive=True)
        assert excl and incl
        assert not any(n - 1 in w for n, w in excl)
        assert any(n - 1 in w for n, w in incl), 'inclusive=True never drew the last non-clicked news'


def test_pure_in_seed_epoch_and_record():
    counts = cases.mixed_counts(3000, seed=4)
    base = counter_negative_draws(counts, K, 5, 1)
    assert np.array_equal(base, counter_negative_draws(counts, K, 5, 1))
    assert not np.array_equal(base, counter_negative_draws(counts, K, 5, 2))
    assert not np.array_equal(base, counter_negative_draws(counts, K, 6, 1))
    assert np.array_equal(base[:1234], counter_negative_draws(counts[:1234], K, 5, 1))
    assert np.array_equal(base[:, :2][counts <= 2], counter_negative_draws(counts, 2, 5, 1)[counts <= 2])
    beh = cases.records(counts[:500])
    full = counter_negative_sampling(beh, K, 5, 1)
    part = counter_negative_sampling(beh[:200], K, 5, 1)
    assert all(a[:200] == b for a, b in zip(full, part))
    assert full == counter_negative_sampling(beh, K, 5, 1) and full != counter_negative_sampling(beh, K, 5, 2)


def chi2(positions, cells):
    counts = np.bincount(positions, minlength=cells)
    assert counts.size == cells
    e = positions.size / cells
    return float(((counts - e) ** 2 / e).sum())


def test_distribution_matches_the_reference_rule():
    """N = 20,000 records of n = 12, K = 4: per slot the chi-square of the drawn position over the 11 reachable ones stays under the
    0.999 quantile (10 degrees of freedom).  Everything is seeded, so the figures are fixed: this is a check of the rule, not a
    coin toss.  The reference's own draw-and-reject loop under numpy.random is held to the same bound first: it is the yardstick."""
    N, n = 20000, 12
    # seed 0 of numpy.random: the reference's rule gives 14.0, 2.1, 5.8 and 8.0 there (the first seed tried; a seed for which the
    # yardstick itself fails its bound -- about one in 250 would, with four slots at 0.999 each -- could not be used)
    np.random.seed(0)
    beh = [[0, None, None, 1, list(range(n)), i, 1.0, 2.0, [float(x) for x in range(n)]] for i in range(N)]
    ref = np.asarray(negative_sampling(beh, K)[0])[:, 1:]
    assert ref.max() == n - 2
    ref_stats = [chi2(ref[:, j], n - 1) for j in range(K)]
    print('reference rule, numpy seed 0: chi-square per slot', ref_stats)
    assert max(ref_stats) < CHI2_10DF_999

    d = counter_negative_draws(np.full(N, n), K, seed=7, epoch=1)
    assert d.min() == 0 and d.max() == n - 2, 'index n - 1 must never be drawn'
    assert all(len(set(row)) == K for row in d.tolist())
    stats = [chi2(d[:, j], n - 1) for j in range(K)]
    print('counter-based rule, seed 7 epoch 1: chi-square per slot', stats)
    assert max(stats) < CHI2_10DF_999

    d = counter_negative_draws(np.full(N, K + 1), K, seed=7, epoch=1)            # n = K + 1: every row a permutation of 0 .. K - 1
    assert np.array_equal(np.sort(d, axis=1), np.tile(np.arange(K), (N, 1)))
    first = chi2(d[:, 0], K)
    print('n = K + 1: chi-square of the first slot', first)
    assert first < CHI2_3DF_999


def test_a_record_without_non_clicked_news_is_named():
    beh = cases.records([3, 5, 9, 2])
    beh[2][4], beh[2][8] = [], []
    with pytest.raises(ValueError, match=r'record 2\b'):
        counter_negative_sampling(beh, K, 0, 1)
    with pytest.raises(ValueError, match=r'record 2\b'):
        counter_negative_draws([4, 7, 0, 1], K, 0, 1)
    with pytest.raises(ValueError):
        counter_negative_draws([4, 7], 0, 0, 1)
    with pytest.raises(ValueError):
        counter_negative_draws([4, 7], _lib.NEG_MAX_K + 1, 0, 1)


def test_entry_point_refuses_bad_arguments_without_a_launch():
    build_library()
    lib = _lib.load()
    fn = lib.lime_negative_sample
    assert fn(None, None, None, 0, None, None, None, None, None, None, 4, K, 0, 1, 0, None) == -1
    assert b'NULL' in lib.lime_last_error_string()
    buf = ctypes.create_string_buffer(64)                          # never read: every call below is refused before a launch
    p = ctypes.c_void_p(ctypes.addressof(buf))
    assert fn(p, p, p, 0, p, p, p, p, p, None, 1, K, 0, 1, 0, None) == -1
    assert fn(p, p, p, 4, p, p, p, p, p, p, 1, 0, 0, 1, 0, None) == -1
    assert b'K 0' in lib.lime_last_error_string()
    assert fn(p, p, p, 4, p, p, p, p, p, p, 1, _lib.NEG_MAX_K + 1, 0, 1, 0, None) == -1
    assert fn(p, p, p, 4, p, p, p, p, p, p, 1, -3, 0, 1, 0, None) == -1
    assert fn(p, p, p, 2 ** 31, p, p, p, p, p, p, 1, K, 0, 1, 0, None) == -1
    assert fn(p, p, p, 4, p, p, p, p, p, p, -1, K, 0, 1, 0, None) == -1
    assert fn(p, p, p, 4, p, p, p, p, p, p, 0, K, 0, 1, 0, None) == 0           # no record: nothing to launch


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 14
    assert 'lime_negative_sample' in _lib.SIGNATURES and _lib.NEG_MAX_K == 16


def test_ops_wrapper_refuses_cpu_tensors():
    import torch
    from lime_cikm25_amd import ops
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.negative_sample(torch.zeros(4, dtype=torch.int64), z, z.float(), z, z.float(), z.float(), K, 0, 1)
