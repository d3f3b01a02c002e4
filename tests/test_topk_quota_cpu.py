"""The topic quota of the recommended slates without a GPU: ``recommend.quota_topk`` (the host statement that every device test is
held against) against a literal sequential walk; the chunked form that the kernel rests on -- every chunk cut to the head of its OWN
walk, the merged lists walked again, several rounds -- against the global walk; the C ABI's refusals; the Python-level refusals of the
three Model entries."""
import ctypes
import subprocess
import types

import numpy as np
import pytest
import torch

from lime_cikm25_amd import Model, _lib, make_config, recommend
from lime_cikm25_amd.build import build_library
from quota_cases import TOPK_MAX, crowded, drop_mask, edge_rows, group_keys, sequential_walk
from user_cases import _TINY


def walk_rows(scores, keys, k, quota, drop=None):
    U = scores.shape[0]
    pos = np.full((U, k), -1, dtype=np.int32)
    top = np.full((U, k), -np.inf, dtype=np.float32)
    for u in range(U):
        taken = sequential_walk(scores[u], keys, k, quota, None if drop is None else drop[u % drop.shape[0]])
        pos[u, :len(taken)] = taken
        top[u, :len(taken)] = scores[u, taken]
    return pos, top


@pytest.mark.parametrize('C', [1, 2, 37, 300])
@pytest.mark.parametrize('k,quota', [(1, 1), (10, 1), (10, 2), (10, 10), (128, 3)])
def test_quota_topk_is_the_sequential_walk(C, k, quota):
    scores, keys = edge_rows(5, C, seed=C + k), group_keys(C, 6, seed=C)
    keys[::11] = -1                                                          # a key outside the table: dropped
    for drop in (None, drop_mask(5, C, seed=1), drop_mask(2, C, seed=2)):    # (two mask rows for five score rows: the schedule view)
        got = recommend.quota_topk(scores, keys, k, quota, drop)
        want = walk_rows(scores, keys, k, quota, drop)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


def test_quota_topk_on_random_small_cases_with_ties():
    rng = np.random.default_rng(0)
    values = np.array([0.0, -0.0, 1.0, 2.0, -1.0, np.nan, -np.inf, 3.0], dtype=np.float32)
    for _ in range(1500):
        C, k, quota = int(rng.integers(1, 50)), int(rng.integers(1, 12)), int(rng.integers(1, 5))
        scores = rng.choice(values, size=(2, C))
        keys = rng.integers(-1, 5, size=C)
        drop = rng.random((2, C)) < 0.2
        got, want = recommend.quota_topk(scores, keys, k, quota, drop), walk_rows(scores, keys, k, quota, drop)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


def test_a_binding_quota_changes_the_slate_and_a_loose_one_does_not():
    scores = np.array([[9, 8, 7, 6, 5, 4, 3]], dtype=np.float32)
    keys = np.array([0, 0, 0, 1, 0, 1, 2])
    assert recommend.quota_topk(scores, keys, 4, 2)[0].tolist() == [[0, 1, 3, 5]]
    assert recommend.quota_topk(scores, keys, 4, 4)[0].tolist() == [[0, 1, 2, 3]]
    assert recommend.quota_topk(scores, keys, 5, 1)[0].tolist() == [[0, 3, 6, -1, -1]]
    assert recommend.quota_topk(scores, keys, 3, 1, drop=np.array([[1, 0, 0, 0, 0, 0, 0]]))[0].tolist() == [[1, 3, 6]]   # no quota used by 0


def test_segment_form_counts_positions_within_the_segment():
    scores = np.array([5, 4, 3, 9, 8, 7, 6], dtype=np.float32)
    keys = np.array([0, 0, 1, 2, 2, 2, 0])
    pos, top = recommend.quota_topk_segments(scores, [0, 3, 3, 7], keys, 3, 1)
    assert pos.tolist() == [[0, 2, -1], [-1, -1, -1], [0, 3, -1]] and top[2].tolist()[:2] == [9.0, 6.0] and np.isneginf(top[1]).all()


# ---- the chunked form: fact 2 of csrc/topk_quota_f32.hip ------------------------------------------------------------------------------
def chunked_walk(row, keys, k, quota, drop, chunk, limit, per):
    """Every chunk of `chunk` entries cut to the first `limit` of its OWN walk; then rounds: the survivors so far beside `per` chunk
    lists, walked again, cut to `limit`; the first k of the last round."""
    def walk_of(positions, n):
        positions = np.sort(np.asarray(positions, dtype=np.int64))
        taken = sequential_walk(row[positions], keys[positions], n, quota, None if drop is None else drop[positions])
        return positions[taken].tolist()
    lists = [walk_of(np.arange(c0, min(len(row), c0 + chunk)), limit) for c0 in range(0, len(row), chunk)]
    best = []
    for c in range(0, len(lists), per):
        best = walk_of(best + [p for l in lists[c:c + per] for p in l], limit)
    return best[:k]


@pytest.mark.parametrize('chunk,limit,per', [(16, 8, 3), (7, 5, 2), (50, 12, 1), (4096, TOPK_MAX, 31)])
def test_chunked_walk_equals_the_global_walk(chunk, limit, per):
    rng = np.random.default_rng(chunk + limit)
    values = np.array([0.0, -0.0, 1.0, 2.0, 3.0, -1.0, np.nan, -np.inf], dtype=np.float32)
    for case in range(3 if chunk == 4096 else 400):
        C = 3 * chunk + 17 if chunk == 4096 else int(rng.integers(1, 12 * chunk))
        row = rng.choice(values, size=C) if case % 2 else rng.standard_normal(C).astype(np.float32)
        keys = np.minimum(rng.integers(0, 6, size=C), rng.integers(0, 6, size=C))          # skewed towards group 0
        drop = rng.random(C) < 0.1 if case % 3 == 0 else None
        k, quota = int(rng.integers(1, limit + 1)), int(rng.integers(1, 4))
        assert chunked_walk(row, keys, k, quota, drop, chunk, limit, per) == sequential_walk(row, keys, k, quota, drop), (case, C, k, quota)


def test_filtering_after_the_cut_is_wrong_on_crowded_chunks():
    """What the crowded case of the GPU test is for: the plain best 128 of each chunk hold one group only."""
    scores, keys = crowded()
    want = sequential_walk(scores[0], keys, 10, 2)
    assert (keys[want] == 0).sum() == 2 and len(want) == 10
    head = np.argsort(-scores[0, :4096], kind='stable')[:TOPK_MAX]
    assert (keys[head] == 0).all()
    assert chunked_walk(scores[0], keys, 10, 2, None, 4096, TOPK_MAX, 31) == want


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ('lime_topk_rows_quota_workspace', 'lime_topk_rows_quota_f32', 'lime_topk_segments_quota_workspace', 'lime_topk_segments_quota_f32')


@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    header = open(_lib.HEADER_PATH).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NEW:
        assert name + '(' in header
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert (' T ' + name + '\n') in exported


def test_new_entries_refuse_bad_arguments_without_a_launch(lib):
    one = ctypes.c_void_p(16)                       # a non-NULL, 16-byte aligned address: never dereferenced by a refused call
    ws = lib.lime_topk_rows_quota_workspace
    assert ws(0, 9000) == 0 and ws(3, 4096) == 0 and ws(3, 4097) == 3 * 2 * 128 * 2 == lib.lime_topk_rows_workspace(3, 4097)

    def rows(U=3, C=10, ld=10, keys=one, n_keys=8, quota=2, drop=None, drop_rows=0, k=4, w=one, n=1 << 30):
        return lib.lime_topk_rows_quota_f32(one, ld, U, C, keys, n_keys, quota, drop, drop_rows, k, one, one, w, n, None)
    assert rows(keys=None) == -1 and b'NULL' in lib.lime_last_error_string()
    assert rows(ld=9) == -1 and rows(C=0, ld=0) == -1 and rows(U=-1) == -1
    assert rows(quota=0) == -1 and b'quota' in lib.lime_last_error_string()
    assert rows(n_keys=0) == -1 and rows(drop=one, drop_rows=0) == -1
    assert rows(n_keys=8193) == -2 and b'8192' in lib.lime_last_error_string()
    assert rows(k=0) == -2 and rows(k=129) == -2 and rows(U=65536) == -2
    assert rows(C=5000, ld=5000, w=None, n=0) == -1 and b'lime_topk_rows_quota_workspace()' in lib.lime_last_error_string()
    assert rows(C=5000, ld=5000, n=3 * 2 * 256 - 1) == -1                                               # one float short
    assert rows(C=5000, ld=5000, w=ctypes.c_void_p(20)) == -1                                           # misaligned
    assert rows(U=0) == 0                                                                               # no rows: nothing to do
    ws = lib.lime_topk_segments_quota_workspace
    assert ws(0, 100) == 0 and ws(3, 0) == 8 and ws(3, 4096) == 8 + 2 * 128 * 2 == lib.lime_topk_segments_workspace(3, 4096)

    def segs(U=3, P=10, keys=one, n_keys=8, quota=2, k=4, w=one, n=1 << 30):
        return lib.lime_topk_segments_quota_f32(one, one, U, P, keys, n_keys, quota, None, k, one, one, w, n, None)
    assert segs(keys=None) == -1 and b'NULL' in lib.lime_last_error_string()
    assert segs(U=-1) == -1 and segs(P=-1) == -1 and segs(quota=0) == -1 and segs(n_keys=0) == -1
    assert segs(n_keys=8193) == -2 and b'8192' in lib.lime_last_error_string()
    assert segs(k=0) == -2 and segs(k=129) == -2
    assert segs(w=None, n=0) == -1 and b'lime_topk_segments_quota_workspace()' in lib.lime_last_error_string()
    assert segs(n=7) == -1 and segs(w=ctypes.c_void_p(20), n=8) == -1
    assert segs(U=0, P=0) == 0


# ---- the Model entries ---------------------------------------------------------------------------------------------------------------
def users(U=3, H=6, n_news=20):
    return dict(news_cache=torch.zeros(n_news, 8), corpus=None, hist_index=torch.zeros(U, H, dtype=torch.int32),
                hist_mask=torch.ones(U, H, dtype=torch.bool), user_freshness=torch.zeros(U, H), user_lifetime=torch.zeros(U, H))


def entries(model, U=3, C=5, **more):
    pool = dict(users(U), cand_index=torch.arange(C, dtype=torch.int32), cand_freshness=torch.zeros(C), cand_lifetime=torch.zeros(U, C), k=2)
    lists = dict(users(U), cand_offsets=torch.tensor([0, 2, 2, C]), cand_index=torch.arange(C, dtype=torch.int32),
                 cand_freshness=torch.zeros(C), cand_lifetime=torch.zeros(C), k=2)
    return [lambda **kw: model.recommend(**{**pool, **more, **kw}),
            lambda **kw: model.recommend_schedule(slot_offsets=torch.zeros(2), **{**pool, **more, **kw}),
            lambda **kw: model.recommend_lists(**{**lists, **more, **kw})]


@pytest.mark.parametrize('bad', [0, -1, 2.0, '2', True])
def test_max_per_topic_must_be_an_integer_of_one_at_least(bad):
    model = Model(make_config(**_TINY))
    for entry in entries(model):
        with pytest.raises(ValueError, match='max_per_topic must be an integer >= 1'):
            entry(max_per_topic=bad)


def test_unknown_quota_by_is_refused():
    model = Model(make_config(**_TINY))
    for entry in entries(model):
        with pytest.raises(ValueError, match="quota_by must be 'category' or 'topic'"):
            entry(max_per_topic=2, quota_by='subCategory')
        with pytest.raises(ValueError, match='quota_by must be'):
            entry(max_per_topic=2, quota_by=None)


def test_a_corpus_of_more_than_8192_groups_is_refused():
    n = 8193
    corpus = types.SimpleNamespace(news_category=torch.arange(n, dtype=torch.int32), news_subCategory=torch.zeros(n, dtype=torch.int32))
    model = Model(make_config(**_TINY))
    for entry in entries(model, corpus=corpus):
        with pytest.raises(ValueError, match='8193 groups by category.*8192'):
            entry(max_per_topic=2)


def test_without_a_quota_the_old_refusals_come_first_and_quota_by_is_not_read():
    model = Model(make_config(**_TINY))
    for entry in entries(model):
        with pytest.raises(ValueError, match='pairs_per_pass must be positive'):
            entry(pairs_per_pass=0, quota_by='anything')
