"""Pool recommendation without a GPU: the host grouping plan (lime_cikm25_amd.recommend), the host-side refusals of Model.score_pool /
Model.recommend, and the two new entries of the C ABI (header, binding, the built library's exports, their argument refusals)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from lime_cikm25_amd import Model, make_config, recommend, _lib
from lime_cikm25_amd.build import build_library

from user_cases import _TINY


# ---- the grouping plan ---------------------------------------------------------------------------------------------------------------
CAT = [3, 1, 3, 2, 1, 3, 1]
SUB = [7, 4, 5, 9, 4, 7, 2]


def test_plan_sorts_by_topic_and_keeps_position_order_inside_a_group():
    p = recommend.pool_plan(CAT, SUB, 'topic')
    # topics ascending by (category, subCategory): (1, 2) (1, 4) (2, 9) (3, 5) (3, 7)
    assert p.category.tolist() == [1, 1, 2, 3, 3] and p.subCategory.tolist() == [2, 4, 9, 5, 7]
    assert p.order.tolist() == [6, 1, 4, 3, 2, 0, 5]
    assert p.segments.tolist() == [0, 1, 3, 4, 5, 7]
    assert p.order.dtype == np.int64 and p.segments.dtype == np.int64
    for t in range(5):
        members = p.order[p.segments[t]:p.segments[t + 1]]
        assert all(CAT[j] == p.category[t] and SUB[j] == p.subCategory[t] for j in members)
        assert members.tolist() == sorted(members.tolist())


def test_plan_by_category_ignores_the_subcategory():
    p = recommend.pool_plan(CAT, SUB, 'category')
    assert p.category.tolist() == [1, 2, 3]
    assert p.order.tolist() == [1, 4, 6, 3, 0, 2, 5] and p.segments.tolist() == [0, 3, 4, 7]


def test_plan_without_the_attention_is_one_group_in_pool_order():
    p = recommend.pool_plan(CAT, SUB, None)
    assert p.order.tolist() == list(range(7)) and p.segments.tolist() == [0, 7] and p.category.shape == (1,)
    # ... and so one group per user
    assert recommend.group_offsets(p.segments, 3).tolist() == [0, 7, 14, 21]


def test_plan_with_given_topics_keeps_empty_groups():
    topics = [(3, 7), (5, 5), (1, 4), (1, 2), (2, 9), (3, 5), (0, 0)]
    p = recommend.pool_plan(CAT, SUB, 'topic', topics=topics)
    assert p.category.tolist() == [t[0] for t in topics] and p.subCategory.tolist() == [t[1] for t in topics]
    assert p.segments.tolist() == [0, 2, 2, 4, 5, 6, 7, 7]                     # (5, 5) and (0, 0) have no candidate: empty, kept
    assert p.order.tolist() == [0, 5, 1, 4, 6, 3, 2]
    with pytest.raises(ValueError, match='not in topics'):
        recommend.pool_plan(CAT, SUB, 'topic', topics=topics[1:])
    with pytest.raises(ValueError, match='twice'):
        recommend.pool_plan(CAT, SUB, 'topic', topics=topics + [(3, 7)])


def test_group_offsets_are_user_major_csr():
    p = recommend.pool_plan(CAT, SUB, 'topic')
    off = recommend.group_offsets(p.segments, 3)
    T, C = 5, 7
    assert off.dtype == np.int64 and off.shape == (3 * T + 1,)
    for u in range(3):
        for t in range(T):
            assert off[u * T + t] == u * C + p.segments[t]
    assert off[-1] == 3 * C and (np.diff(off) >= 0).all()
    assert recommend.group_offsets(p.segments, 0).tolist() == [0]
    with pytest.raises(ValueError):
        recommend.group_offsets([1, 2], 1)


def test_plan_refuses_bad_input():
    with pytest.raises(ValueError):
        recommend.pool_plan([], [], 'topic')
    with pytest.raises(ValueError):
        recommend.pool_plan([1, 2], [1], 'topic')
    with pytest.raises(ValueError):
        recommend.pool_plan([1], [1], 'subcategory')


def test_users_per_pass_bounds_both_row_counts():
    assert recommend.users_per_pass(32, 65536, 300, 50, 1 << 18) == 4           # 4 x 65536 candidate rows
    assert recommend.users_per_pass(32, 2000, 300, 50, 1 << 18) == 16           # 17 x 300 x 50 refined rows at the most, evened: 2 passes
    assert recommend.users_per_pass(3, 37, 5, 6, 40) == 1                       # one user at the least
    assert recommend.users_per_pass(5, 10, 1, 2, 1 << 18) == 5
    with pytest.raises(ValueError):
        recommend.users_per_pass(3, 37, 5, 6, 0)


# ---- host-side refusals --------------------------------------------------------------------------------------------------------------
def pool_args(U=3, H=6, C=5, n_news=20):
    return dict(news_cache=torch.zeros(n_news, 8), corpus=None, hist_index=torch.zeros(U, H, dtype=torch.int32),
                hist_mask=torch.ones(U, H, dtype=torch.bool), user_freshness=torch.zeros(U, H), user_lifetime=torch.zeros(U, H),
                cand_index=torch.arange(C, dtype=torch.int32), cand_freshness=torch.zeros(C), cand_lifetime=torch.zeros(U, C))


def test_cne_is_refused_before_anything_else():
    model = Model(make_config(content_encoder='CNE', **_TINY))
    with pytest.raises(ValueError, match='CNE.*no per-news content cache'):
        model.score_pool(**pool_args())
    with pytest.raises(ValueError, match='CNE.*no per-news content cache'):
        model.recommend(k=2, **pool_args())


@pytest.mark.parametrize('change,match', [
    (dict(hist_index=torch.zeros(3, dtype=torch.int32)), r'hist_index must be \[U, H\]'),
    (dict(hist_mask=torch.ones(3, 5, dtype=torch.bool)), 'hist_mask must be'),
    (dict(user_lifetime=torch.zeros(2, 6)), 'user_lifetime must be'),
    (dict(cand_index=torch.zeros(3, 5, dtype=torch.int32)), 'ONE pool for all users'),
    (dict(cand_index=torch.zeros(0, dtype=torch.int32)), 'ONE pool for all users'),
    (dict(cand_index=torch.zeros(5)), 'int32 or int64'),
    (dict(cand_freshness=torch.zeros(4)), 'cand_freshness must be'),
    (dict(cand_lifetime=torch.zeros(5, 3)), 'cand_lifetime must be'),
    (dict(news_cache=torch.zeros(20, 0)), 'news_cache must be'),
    (dict(pairs_per_pass=0), 'pairs_per_pass must be positive'),
])
def test_bad_shapes_are_value_errors_on_the_host(change, match):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match=match):
        model.score_pool(**dict(pool_args(), **change))
    with pytest.raises(ValueError, match=match):
        model.recommend(k=1, **dict(pool_args(), **change))


@pytest.mark.parametrize('k', [0, -1, 129])
def test_k_out_of_range_is_a_value_error(k):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match='1 <= k <= 128'):
        model.recommend(k=k, **pool_args())


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ('lime_grouped_match_f32', 'lime_topk_rows_f32', 'lime_topk_rows_workspace')


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
    assert lib.lime_abi_version() == 14 == _lib.ABI_VERSION


def test_new_entries_refuse_bad_arguments_without_a_launch(lib):
    one = ctypes.c_void_p(16)                       # a non-NULL, 16-byte aligned address: never dereferenced by a refused call
    gm = lambda H, A, D, kp=one: lib.lime_grouped_match_f32(kp, one, one, one, None, one, one, 1, 1, H, A, D, 1.0, 0.0, 0.0, 0, 0, None)
    assert gm(4, 8, 8, kp=None) == -1 and b'NULL' in lib.lime_last_error_string()
    for H, A, D in ((0, 8, 8), (4, 0, 8)):
        assert gm(H, A, D) == -1
    for H, A, D in ((129, 8, 8), (4, 2052, 8), (4, 8, 2052), (4, 6, 8), (4, 8, 10)):
        assert gm(H, A, D) == -2, (H, A, D)
        msg = lib.lime_last_error_string()
        assert b"128" in msg and b"2048" in msg and b'multiples of 4' in msg
    assert lib.lime_grouped_match_f32(ctypes.c_void_p(20), one, one, one, None, one, one, 1, 1, 4, 8, 8, 1.0, 0.0, 0.0, 0, 0, None) == -1
    assert lib.lime_grouped_match_f32(one, one, one, one, None, one, one, 1, 1, 4, 8, 8, 1.0, 0.0, 0.0, 1, 0, None) == -1   # weight without remaining
    tk = lambda U, C, k, ld=None, ws=None, n=0: lib.lime_topk_rows_f32(one, C if ld is None else ld, U, C, k, one, one, ws, n, None)
    assert tk(1, 0, 1) == -1 and tk(1, 8, 1, ld=7) == -1
    assert tk(1, 8, 0) == -2 and tk(1, 8, 129) == -2 and tk(65536, 8, 1) == -2
    assert lib.lime_topk_rows_workspace(3, 4096) == 0 and lib.lime_topk_rows_workspace(3, 4097) == 3 * 2 * 128 * 2
    assert lib.lime_topk_rows_workspace(2, 1 << 20) == 2 * 256 * 128 * 2
    assert tk(3, 4097, 4) == -1 and b'lime_topk_rows_workspace()' in lib.lime_last_error_string()       # no workspace
    assert tk(3, 4097, 4, ws=one, n=3 * 2 * 128 * 2 - 1) == -1                                          # one float short
    assert tk(3, 4097, 4, ws=ctypes.c_void_p(20), n=3 * 2 * 128 * 2) == -1                              # misaligned
    assert tk(0, 8, 1) == 0                                                                             # no rows: nothing to do
