"""Slate evaluation, host part (CPU only): recommend.slate_metrics -- the numpy statement of what csrc/slate_metrics.hip computes -- on
hand-worked slates and against evaluate.metrics_from_ranks on the plain top k, and the refusals of ops.slate_metrics,
util.evaluate_slates_on_device and Trainer(slate_eval=...), which must come before anything is launched."""
import ctypes
import types

import numpy as np
import pytest
import torch

from lime_cikm25_amd import _lib, evaluate as E, ops, recommend
from lime_cikm25_amd import util as U
from slate_cases import host_metrics, ragged_case, slate_case

D = 1.0 / np.log2(np.arange(8) + 2.0)             # the discounts: 1, 1 / log2(3), 1 / 2, ..
# six news: a zero row, e0, e1, e0 + e1, 2 e0, -e0
TABLE = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [2, 0, 0, 0], [-1, 0, 0, 0]], dtype=np.float32)
KEYS = np.array([0, 1, 1, 2, 1, 3])


def lists(*parts):
    """(news, labels) lists -> offsets, news, labels of the CSR."""
    off = np.concatenate([[0], np.cumsum([len(n) for n, _ in parts])])
    return off, np.concatenate([n for n, _ in parts]), np.concatenate([y for _, y in parts])


def test_hand_worked_relevance_columns():
    off, news, labels = lists(([1, 2, 3, 4], [1, 0, 0, 0]),          # a positive in slot 0
                              ([1, 2, 3, 4], [0, 0, 1, 0]),          # ... in the last slot
                              ([1, 2, 3, 4], [0, 0, 0, 1]),          # ... nowhere in the slate
                              ([1, 2], [0, 1]),                      # a list shorter than k: a trailing -1
                              ([1, 2, 3], [0, 1, 0]),                # a -1 in the middle keeps its slot
                              ([1, 2, 3], [1, 1, 1]),                # one class only
                              ([1, 2, 3], [0, 2, 1]),                # a label outside {0, 1}
                              ([], []),                              # no rows
                              ([1, 2, 3], [1, 0, 1]))                # skipped
    pos = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2], [1, 0, -1], [0, -1, 1], [0, 1, 2], [0, 1, 2], [-1, -1, -1], [0, 1, 2]])
    skip = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1])
    per, status, sums, counts = recommend.slate_metrics(pos, 3, off, news, labels, skip, None, TABLE, KEYS)
    assert status.tolist() == [0, 0, 0, 0, 0, 2, 3, 1, 1]
    assert per[0, :4].tolist() == [1.0, 1.0, 1.0, 1.0]
    assert per[1, :4].tolist() == [D[2] / D[0], 1.0 / 3.0, 1.0, 1.0]
    assert per[2, :4].tolist() == [0.0, 0.0, 0.0, 0.0]
    assert per[3, :4].tolist() == [1.0, 1.0, 1.0, 1.0] and per[3, 6] == 2
    assert per[4, :4].tolist() == [D[2] / D[0], 1.0 / 3.0, 1.0, 1.0] and per[4, 6] == 2      # the positive sits in slot 2, not 1
    assert (per[5:, :4] == 0).all()
    # diversity: cos(e0, e1) = 0, cos(e0, e0 + e1) = cos(e1, e0 + e1) = 1 / sqrt 2
    assert abs(per[0, 4] - (1.0 - np.sqrt(2.0) / 3.0)) < 1e-15
    assert per[3, 4] == 1.0 and per[4, 4] == 1.0
    assert per[:, 5].tolist() == [2, 2, 2, 1, 1, 2, 2, 0, 2]        # keys 1, 1, 2
    assert per[7].tolist() == [0.0] * 8
    assert counts.tolist() == [5, 7, 7]                              # the skipped slate feeds nothing, the empty one no diversity set
    assert sums[0] == per[:5, 0].sum() and sums[6] == per[:7, 6].sum() and sums[4] == per[:7, 4].sum()


def test_hand_worked_more_positives_than_slots():
    off, news, labels = lists(([1, 2, 3, 4, 5], [1, 1, 1, 0, 1]))
    per, status, _, _ = recommend.slate_metrics([[0, 3]], 2, off, news, labels)
    assert status.tolist() == [0]
    assert per[0, :4].tolist() == [D[0] / (D[0] + D[1]), 1.0, 1.0, 0.25]
    per, _, _, _ = recommend.slate_metrics([[3, 1]], 2, off, news, labels)
    assert per[0, :4].tolist() == [D[1] / (D[0] + D[1]), 0.5, 1.0, 0.25]


def test_hand_worked_diversity_columns():
    off, news, _ = lists(([4, 1], []), ([1, 1], []), ([0, 1], []), ([1, 5], []), ([1, 2], []))
    pos = np.array([[0, 1], [0, 1], [0, 1], [0, 1], [0, -1]])
    value = np.array([1.5, 2.5, 0, 0, 0, 0, 7, 9, 3, 4], dtype=np.float32)
    per, status, sums, counts = recommend.slate_metrics(pos, 2, off, news, None, None, value, TABLE, KEYS)
    assert status.tolist() == [1] * 5 and (per[:, :4] == 0).all()    # no labels: nothing is counted for relevance
    assert per[0, 4] == 0.0                                          # 2 e0 and e0: cos 1
    assert per[1, 4] == 0.0                                          # one news twice
    assert per[2, 4] == 1.0                                          # a zero row: cos 0
    assert per[3, 4] == 2.0                                          # e0 and -e0: cos -1
    assert per[4, 4] == 0.0 and per[4, 6] == 1                       # one filled slot: no pair
    assert per[:, 5].tolist() == [1, 1, 2, 2, 1]
    assert per[:, 7].tolist() == [2.0, 0.0, 0.0, 8.0, 3.0]
    assert counts.tolist() == [0, 4, 5] and sums[4] == 3.0 and sums[7] == 13.0
    # a pool: every slate indexes the same rows
    per, _, _, counts = recommend.slate_metrics([[0, 1], [1, 3], [9, 12]], 2, None, news, table=TABLE)
    assert per[:, 4].tolist() == [0.0, 0.0, 0.0] and per[:, 6].tolist() == [2, 2, 1] and counts.tolist() == [0, 2, 3]
    # a news id outside the table is an empty slot
    per, _, _, _ = recommend.slate_metrics([[0, 1, 2]], 3, None, [1, 9, 2], table=TABLE, keys=KEYS)
    assert per[0, 4:7].tolist() == [1.0, 1.0, 2.0]
    with pytest.raises(ValueError, match='labels need offsets'):
        recommend.slate_metrics([[0]], 1, None, [1], labels=[1])
    with pytest.raises(ValueError):
        recommend.slate_metrics([[0]], 2, None, [1])


def top_k_slates(scores, indices, n_imp, k):
    """The plain top k of every impression by recommend.walk_order's stable rule -> (positions [n_imp, k], offsets)."""
    off = np.searchsorted(np.asarray(indices), np.arange(n_imp + 1), side='left')
    pos = np.full((n_imp, k), -1, dtype=np.int32)
    for i in range(n_imp):
        order = recommend.walk_order(scores[off[i]:off[i + 1]])[:k]
        pos[i, :order.size] = order
    return pos, off


@pytest.mark.parametrize('seed', [0, 1])
def test_plain_top_k_reproduces_the_ndcg_of_the_rank_metrics(seed):
    scores, indices, labels = ragged_case(seed, n_imp=200)
    labels[7], labels[11] = [], [1] * len(labels[11])                # a label-less truth line, one class only
    labels[13][0] = 2
    ranks = U.rank_impressions(scores, indices)
    want, want_status = E.metrics_from_ranks(ranks, labels, per_impression=True)
    _, row_labels, skip = E.impression_layout(indices, labels)
    for k, col in ((5, 2), (10, 3)):
        pos, off = top_k_slates(np.asarray(scores, dtype=np.float32), indices, len(labels), k)
        per, status, sums, counts = recommend.slate_metrics(pos, k, off, np.zeros(len(scores), dtype=np.int64), row_labels, skip)
        assert status.tolist() == want_status.tolist() and sorted(set(status.tolist())) == [0, 1, 2, 3]
        ok = status == 0
        print('nDCG@%d, slate - rank metrics: max %.3e' % (k, np.abs(per[ok, 0] - want[ok, col]).max()))
        assert np.array_equal(per[ok, 0], want[ok, col])
        assert counts[0] == ok.sum() and (per[~ok, :4] == 0).all()
        # RR@k is the reciprocal rank of the best positive where it made the slate
        best = np.array([min((q for q, y in zip(r, l) if y), default=10 ** 9) if l else 10 ** 9 for r, l in zip(ranks, labels)])
        assert np.array_equal(per[ok, 1], np.where(best[ok] <= k, 1.0 / best[ok], 0.0))


def test_generated_cases_hold_what_they_promise():
    c = slate_case(3, R=257, k=10, ldp=13, E=8, n=50, n_keys=7, lens=[1, 4, 299])
    per, status, sums, counts = host_metrics(c)
    assert sorted(set(status.tolist())) == [0, 1, 2, 3]
    assert (per[:, 6] == 0).any() and (per[:, 6] == 10).any() and (per[:, 6] == 1).any()
    assert counts[0] > 50 and counts[1] < counts[2] < 257
    assert 0.0 < sums[4] / counts[1] < 1.5 and (per[:, 5] <= per[:, 6]).all()
    lo, _, _, _ = host_metrics(c, k=5)                               # a prefix is the slate at the smaller k
    again = dict(c, positions=np.ascontiguousarray(c['positions'][:, :5]), k=5)
    assert np.array_equal(lo, host_metrics(again)[0])


def no_library():
    raise AssertionError('the library was reached: a launch would follow')


def test_ops_slate_metrics_refuses_without_a_launch(monkeypatch):
    monkeypatch.setattr(_lib, 'load', no_library)
    pos, news = torch.zeros((2, 3), dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.slate_metrics(pos, 3, None, news)                        # CPU tensors: the HIP path has no CPU fallback
    with pytest.raises(TypeError):
        ops.slate_metrics([[0, 1]], 2, None, news)
    if torch.cuda.is_available():
        pos, news = pos.cuda(), news.cuda()
        off = torch.tensor([0, 2, 4]).cuda()
        with pytest.raises(ValueError, match='1 <= k'):
            ops.slate_metrics(pos, 4, None, news)
        with pytest.raises(ValueError, match='1 <= k'):
            ops.slate_metrics(pos, 0, None, news)
        with pytest.raises(TypeError):
            ops.slate_metrics(pos.long(), 3, None, news)
        with pytest.raises(ValueError, match='labels need offsets'):
            ops.slate_metrics(pos, 3, None, news, labels=torch.zeros(4, dtype=torch.uint8).cuda())
        with pytest.raises(ValueError):
            ops.slate_metrics(pos, 3, off[:2], news)                 # offsets: R + 1 entries
        with pytest.raises(TypeError):
            ops.slate_metrics(pos, 3, off.int(), news)
        with pytest.raises(TypeError):
            ops.slate_metrics(pos, 3, off.cpu(), news)
        with pytest.raises(ValueError):
            ops.slate_metrics(pos, 3, off, news, labels=torch.zeros(3, dtype=torch.uint8).cuda())
        with pytest.raises(ValueError, match='multiple of 4'):
            ops.slate_metrics(pos, 3, off, news, table=torch.zeros((5, 6)).cuda())
        with pytest.raises(TypeError):
            ops.slate_metrics(pos, 3, off, news, table=torch.zeros((5, 8), dtype=torch.float64).cuda())
        with pytest.raises(ValueError, match='alike'):
            ops.slate_metrics(pos, 3, off, news, table=torch.zeros((5, 8)).cuda(), keys=torch.zeros(6, dtype=torch.int32).cuda())
        with pytest.raises(ValueError):
            ops.slate_metrics(pos, 3, off, news, skip=torch.zeros(3, dtype=torch.uint8).cuda())


def fake_split():
    corpus = types.SimpleNamespace(news_category=torch.tensor([0, 1, 1, 2, 2]), news_subCategory=torch.tensor([0, 3, 4, 3, 3]))
    model = types.SimpleNamespace(reads_content_mask=False, build_news_cache=lambda corpus: no_library())
    return model, types.SimpleNamespace(corpus=corpus, num=3)


@pytest.mark.parametrize('settings,k,value,match', [
    ([{'max_per_topic': 0}], 5, None, 'max_per_topic'),
    ([{}, {'max_per_topic': 2, 'quota_by': 'subtopic'}], 5, None, 'quota_by'),
    ([{'mmr_lambda': 1.5}], 5, None, 'mmr_lambda'),
    ([{'mmr_lambda': 0.5, 'shortlist': 3}], 5, None, 'shortlist'),
    ([{'shortlist': 64}], 5, None, 'mmr_lambda alone'),
    ([{'mmr_lambda': 0.5, 'similarity': torch.zeros((5, 6))}], 5, None, 'similarity'),
    ([{'lambda': 0.5}], 5, None, 'unknown key'),
    ([{'topic_by': 'user'}], 5, None, 'topic_by'),
    ({'max_per_topic': 1}, 5, None, 'list of dicts'),
    ([{}], 0, None, '1 <= k <= 128'),
    ([{}], 129, None, '1 <= k <= 128'),
    ([{}], 5, 'age', 'value'),
    ([{}], 5, torch.zeros(4), 'value'),
])
def test_evaluate_slates_refuses_a_bad_sweep_before_any_scoring(monkeypatch, settings, k, value, match):
    monkeypatch.setattr(_lib, 'load', no_library)
    model, behaviors = fake_split()
    with pytest.raises(ValueError, match=match):
        U.evaluate_slates_on_device(model, behaviors, [0, 0, 1], [[1, 0], [1]], settings, k=k, value=value)


def test_trainer_refuses_slate_eval_without_device_eval(monkeypatch):
    from lime_cikm25_amd.trainer import Trainer
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(ValueError, match='device_eval'):
        Trainer(None, None, None, slate_eval=dict(settings=[{}], k=5))
    with pytest.raises(ValueError, match='slate_eval must be'):
        Trainer(None, None, None, device_eval=True, slate_eval=[{}])
    with pytest.raises(ValueError, match='slate_eval must be'):
        Trainer(None, None, None, device_eval=True, slate_eval=dict(settings=[{}], top=5))


def test_library_refuses_bad_slate_arguments_before_any_launch():
    from lime_cikm25_amd.build import build_library
    build_library()
    lib = _lib.load()
    assert 'lime_slate_metrics_f32' in _lib.SIGNATURES and _lib.ABI_VERSION == 14             # an added entry leaves the version alone
    assert lib.lime_slate_metrics_f32(None, None) == -1
    a = _lib.SlateMetricsArgs()
    assert lib.lime_slate_metrics_f32(ctypes.byref(a), None) == -1 and b'NULL' in lib.lime_last_error_string()
