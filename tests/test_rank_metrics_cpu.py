"""The device-side dev pass, host part (CPU only): evaluate.metrics_from_ranks -- the numpy statement of the closed forms the kernel
csrc/rank_metrics.hip evaluates -- against evaluate.scoring (the restatement of the reference's evaluate.py, pinned by the eval
goldens), and the argument checks of ops.rank_metrics / evaluate.device_scoring, which must refuse before anything is launched."""
import ctypes
import io
import json
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR
from lime_cikm25_amd import _lib, evaluate as E, ops
from lime_cikm25_amd import util as U

ATOL = 1e-12                    # the project's bound for these metrics (tests/test_eval_harness.py)


def golden(name):
    with open(os.path.join(GOLDEN_DIR, name + '.json')) as f:
        return json.load(f)


def truth_of(g):
    return [E.parse_line(line)[1] for line in g['truth_file'].split('\n') if line.strip()]


def files(labels, ranks):
    truth = '\n'.join('%d %s' % (i + 1, str(list(l)).replace(' ', '')) for i, l in enumerate(labels))
    sub = '\n'.join('%d %s' % (i + 1, str(list(r)).replace(' ', '')) for i, r in enumerate(ranks))
    return io.StringIO(truth), io.StringIO(sub)


def ragged_case(seed, n_imp=400, max_rows=299):
    """Seeded ragged impressions with heavy ties (scores rounded to one decimal, +0.0 / -0.0 planted); every impression has at least
    two rows, at least one positive and at least one negative."""
    rng = np.random.default_rng(seed)
    scores, indices, labels = [], [], []
    for i in range(n_imp):
        n = int(rng.integers(2, max_rows + 1))
        s = np.round(rng.normal(size=n), 1).astype(np.float32)
        s[rng.random(n) < 0.1] = 0.0
        s[rng.random(n) < 0.05] = -0.0
        y = (rng.random(n) < rng.choice([0.05, 0.3, 0.7])).astype(np.int64)
        a, b = rng.choice(n, 2, replace=False)
        y[a], y[b] = 1, 0
        assert 0 < y.sum() < n
        scores += s.tolist()
        indices += [i] * n
        labels.append(y.tolist())
    return scores, indices, labels


@pytest.mark.parametrize('name', ['eval_plain', 'eval_ties'])
def test_closed_forms_match_scoring_on_the_goldens(name):
    g = golden(name)
    labels = truth_of(g)
    ranks = U.rank_impressions(g['scores'], g['indices'])
    got = E.metrics_from_ranks(ranks, labels)
    want = E.scoring(io.StringIO(g['truth_file']), io.StringIO(g['rank_file']))
    print(name, 'closed forms - scoring:', np.abs(np.array(got) - np.array(want)).max(), '- golden:', np.abs(np.array(got) - np.array(g['metrics'])).max())
    assert np.allclose(got, want, rtol=0, atol=ATOL)
    assert np.allclose(got, g['metrics'], rtol=0, atol=ATOL)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_closed_forms_match_scoring_on_ragged_impressions_with_ties(seed):
    scores, indices, labels = ragged_case(seed)
    ranks = U.rank_impressions(scores, indices)
    got = E.metrics_from_ranks(ranks, labels)
    want = E.scoring(*files(labels, ranks))
    per, status = E.metrics_from_ranks(ranks, labels, per_impression=True)
    assert (status == 0).all() and per.shape == (len(labels), 4)
    # every impression on its own as well: scoring over a one-impression file is that impression's four metrics
    for i in range(0, len(labels), 7):
        one = E.scoring(*files([labels[i]], [ranks[i]]))
        assert np.allclose(per[i], one, rtol=0, atol=ATOL), i
    print('seed', seed, 'closed forms - scoring:', np.abs(np.array(got) - np.array(want)).max())
    assert np.allclose(got, want, rtol=0, atol=ATOL)


def test_skipped_and_degenerate_impressions():
    labels = [[1, 0, 0], [], [0, 1], [1, 1], [0, 2, 1]]
    ranks = [[2, 1, 3], [1, 2], [1, 2], [1, 2], [3, 1, 2]]
    per, status = E.metrics_from_ranks(ranks, labels, per_impression=True)
    assert status.tolist() == [0, 1, 0, 2, 3]
    assert (per[[1, 3, 4]] == 0).all()
    with pytest.raises(ValueError, match='Only one class'):
        E.metrics_from_ranks(ranks[:4], labels[:4])
    # the skipped impression is left out of the means, exactly as scoring leaves it out (its rank line is consumed)
    got = E.metrics_from_ranks(ranks[:3], labels[:3])
    want = E.scoring(*files(labels[:3], ranks[:3]))
    assert np.allclose(got, want, rtol=0, atol=ATOL)
    with pytest.raises(ValueError):
        E.metrics_from_ranks([[1, 2, 3]], [[1, 0]])


def test_impression_layout():
    off, lab, skip = E.impression_layout([0, 0, 2, 2, 2, 3], [[1, 0], [], [0, 0, 1], []])
    assert off.tolist() == [0, 2, 2, 5, 6] and off.dtype == np.int32
    assert lab.tolist() == [1, 0, 0, 0, 1, 0] and lab.dtype == np.uint8
    assert skip.tolist() == [0, 1, 0, 1]
    with pytest.raises(ValueError, match='non-decreasing'):
        E.impression_layout([0, 1, 0], [[1], [0], []])
    with pytest.raises(ValueError):
        E.impression_layout([0, 0, 1], [[1, 0]])                  # an impression the labels do not hold
    with pytest.raises(ValueError):
        E.impression_layout([0, 0, 0], [[1, 0]])                  # three rows, two labels


def test_ops_rank_metrics_refuses_cpu_tensors_and_bad_offsets_without_a_launch(monkeypatch):
    def no_library():
        raise AssertionError('the library was reached: a launch would follow')
    monkeypatch.setattr(_lib, 'load', no_library)
    s, y = torch.zeros(4), torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(TypeError):
        ops.rank_metrics(s, y, [0, 2, 4])
    with pytest.raises(TypeError):
        ops.rank_metrics([0.0] * 4, y, [0, 2, 4])
    with pytest.raises(ValueError, match='non-decreasing'):
        ops.rank_metrics(s, y, [0, 3, 2, 4])
    with pytest.raises(ValueError, match='end at the row count'):
        ops.rank_metrics(s, y, [0, 2, 5])
    with pytest.raises(ValueError):
        ops.rank_metrics(s, y, [1, 2, 4])
    with pytest.raises(ValueError):
        ops.rank_metrics(s, y, [])
    with pytest.raises(ValueError):
        ops.rank_metrics(s, y, torch.tensor([0.0, 4.0]))
    with pytest.raises(ValueError):
        ops.rank_metrics(s, y, torch.tensor([[0, 4]]))


def test_device_scoring_refuses_cpu_scores_and_bad_indices_without_a_launch(monkeypatch):
    def no_library():
        raise AssertionError('the library was reached: a launch would follow')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(TypeError):
        E.device_scoring(torch.zeros(3), [0, 0, 1], [[1, 0], [1]])
    with pytest.raises(TypeError):
        E.device_scoring([0.0, 1.0, 2.0], [0, 0, 1], [[1, 0], [1]])


def test_ranks_to_lists_is_rank_impressions_layout():
    idx = [0, 0, 2, 2, 2]
    assert U.ranks_to_lists(np.array([2, 1, 3, 1, 2], dtype=np.int32), idx) == [[2, 1], [], [3, 1, 2]]
    assert U.ranks_to_lists(torch.tensor([], dtype=torch.int32), []) == []
    want = U.rank_impressions([0.5, 0.7, 0.1, 0.1, 0.9], idx)
    assert U.ranks_to_lists(np.concatenate([np.asarray(r, dtype=np.int32) for r in want]), idx) == want


def test_library_refuses_a_bad_args_struct_before_any_launch():
    from lime_cikm25_amd.build import build_library
    build_library()
    lib = _lib.load()
    assert lib.lime_rank_metrics(None, None) == -1
    a = _lib.RankMetricsArgs()
    assert lib.lime_rank_metrics(ctypes.byref(a), None) == -1 and b'NULL' in lib.lime_last_error_string()
    a.n_imp = -1
    assert lib.lime_rank_metrics(ctypes.byref(a), None) == -1
    assert lib.lime_rank_metrics_workspace(0) == 0 and lib.lime_rank_metrics_workspace(1) == 40
    assert lib.lime_rank_metrics_workspace(1025) == 80 and lib.lime_rank_metrics_workspace(2 ** 31 - 1) == 40 * 2 ** 21
