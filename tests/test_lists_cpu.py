"""Candidate lists without a GPU: the host statement of the grouping plan (recommend.list_plan, recommend.topic_table), the host-side
refusals of Model.score_lists / Model.recommend_lists and of the grouped dev pass, the empty case, and the new entries of the C ABI."""
import ctypes
import subprocess
import types

import numpy as np
import pytest
import torch

from lime_cikm25_amd import Model, make_config, recommend, util, _lib
from lime_cikm25_amd.build import build_library

from user_cases import _TINY


# ---- list_plan -----------------------------------------------------------------------------------------------------------------------
def check_plan(keys, offsets, plan, S):
    """Every property of a ListPlan, from the definition."""
    keys, offsets = np.asarray(keys, dtype=np.int64), np.asarray(offsets, dtype=np.int64)
    P, U = keys.shape[0], offsets.shape[0] - 1
    order, goff, skey, nd = plan
    assert order.dtype == np.int64 and goff.dtype == np.int64 and skey.dtype == np.int32 and nd.dtype == np.int32
    assert order.shape == (P,) and goff.shape == (U * S + 1,) and skey.shape == (U * S,) and nd.shape == (U,)
    assert sorted(order.tolist()) == list(range(P))                                   # a permutation ...
    assert goff[0] == 0 and goff[-1] == P and (np.diff(goff) >= 0).all()
    for u in range(U):
        lo, hi = offsets[u], offsets[u + 1]
        assert sorted(order[lo:hi].tolist()) == list(range(lo, hi))                   # ... that keeps every user's range
        distinct = sorted(set(keys[lo:hi].tolist()))
        assert nd[u] == len(distinct)
        assert goff[u * S] == lo and goff[(u + 1) * S] == hi
        for s in range(S):
            members = order[goff[u * S + s]:goff[u * S + s + 1]]
            if s < len(distinct):
                assert skey[u * S + s] == distinct[s]                                 # slots ascend by key
                assert len(members) > 0 and (keys[members] == distinct[s]).all()      # every group holds one key
                assert members.tolist() == sorted(members.tolist())                   # stable: list order inside a slot
                assert len(members) == (keys[lo:hi] == distinct[s]).sum()
            else:
                assert len(members) == 0                                              # an unused slot is empty ...
                assert skey[u * S + s] == (distinct[0] if distinct else 0)            # ... and carries a valid key


PLANS = {
    'an_empty_list': ([], [0, 0]),
    'one_pair': ([4], [0, 1]),
    'all_pairs_on_one_key': ([2, 2, 2, 2, 2], [0, 5]),
    'all_keys_distinct': ([5, 1, 4, 0, 3], [0, 5]),
    'more_keys_than_another_user_has_pairs': ([3, 3, 7, 1, 0, 5, 1, 7, 2, 2], [0, 2, 9, 9, 10]),
    'ties_in_list_order': ([1, 0, 1, 0, 1, 0, 2, 2, 0], [0, 4, 9]),
}


@pytest.mark.parametrize('name', list(PLANS))
def test_list_plan_on_hand_made_lists(name):
    keys, offsets = PLANS[name]
    plan = recommend.list_plan(keys, offsets)
    U = len(offsets) - 1
    S = plan.slot_key.shape[0] // U
    distinct = [len(set(keys[offsets[u]:offsets[u + 1]])) for u in range(U)]
    assert S == max(1, max(distinct))
    check_plan(keys, offsets, plan, S)


def test_list_plan_written_out():
    plan = recommend.list_plan([3, 3, 7, 1, 0, 5, 1, 7, 2, 2], [0, 2, 9, 9, 10])
    assert plan.n_distinct.tolist() == [1, 5, 0, 1]
    assert plan.order.tolist() == [0, 1, 4, 3, 6, 8, 5, 2, 7, 9]
    assert plan.group_offsets.tolist() == [0, 2, 2, 2, 2, 2, 3, 5, 6, 7, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10]
    assert plan.slot_key.tolist() == [3, 3, 3, 3, 3, 0, 1, 2, 5, 7, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2]


def test_list_plan_with_more_slots_than_needed():
    keys, offsets = PLANS['more_keys_than_another_user_has_pairs']
    wide = recommend.list_plan(keys, offsets, slots=8)
    check_plan(keys, offsets, wide, 8)
    assert np.array_equal(wide.order, recommend.list_plan(keys, offsets).order)


def test_list_plan_refuses_too_few_slots_and_bad_offsets():
    keys, offsets = PLANS['more_keys_than_another_user_has_pairs']
    with pytest.raises(ValueError, match='5 distinct keys'):
        recommend.list_plan(keys, offsets, slots=4)
    for bad in ([1, 10], [0, 9], [0, 6, 5, 10]):
        with pytest.raises(ValueError):
            recommend.list_plan(keys, bad)
    with pytest.raises(ValueError):
        recommend.list_plan([1, -1], [0, 2])


def test_list_passes_bound_pairs_and_refined_rows():
    off, nd = [0, 37, 46, 47, 47], [5, 1, 1, 0]
    assert recommend.list_passes(off, nd, 6, 1 << 18) == [(0, 4, 5)]
    assert recommend.list_passes(off, nd, 6, 40) == [(0, 1, 5), (1, 4, 1)]            # 37 pairs fill a pass; three users x 1 slot x 6 fit
    assert recommend.list_passes(off, nd, 6, 1) == [(0, 1, 5), (1, 2, 1), (2, 3, 1), (3, 4, 1)]   # one user a pass at the least
    assert recommend.list_passes([0], [], 6, 8) == []
    with pytest.raises(ValueError):
        recommend.list_passes(off, nd, 6, 0)


# ---- topic_table ---------------------------------------------------------------------------------------------------------------------
CAT = [3, 1, 3, 2, 1, 3, 1, 3]
SUB = [7, 4, 5, 9, 4, 7, 2, 5]


@pytest.mark.parametrize('by', ['topic', 'category', None])
def test_topic_table_agrees_with_pool_plan(by):
    topic, cat, sub = recommend.topic_table(CAT, SUB, by)
    assert topic.dtype == np.int32 and cat.dtype == np.int64 and sub.dtype == np.int64 and topic.shape == (len(CAT),)
    p = recommend.pool_plan(CAT, SUB, by)
    group_of = np.empty(len(CAT), dtype=np.int64)
    for t in range(len(p.segments) - 1):
        group_of[p.order[p.segments[t]:p.segments[t + 1]]] = t
    assert np.array_equal(topic, group_of)                                            # the same groups, ids in the plan's key order
    assert np.array_equal(cat, p.category) and cat.shape == sub.shape == (topic.max() + 1,)
    if by == 'topic':
        assert np.array_equal(sub, p.subCategory)
    if by is None:
        assert (topic == 0).all()


def test_topic_table_refuses_bad_input():
    with pytest.raises(ValueError):
        recommend.topic_table([], [], 'topic')
    with pytest.raises(ValueError):
        recommend.topic_table([1], [1], 'subcategory')
    with pytest.raises(ValueError):
        recommend.topic_table([1, -1], [1, 1], 'topic')


# ---- host-side refusals --------------------------------------------------------------------------------------------------------------
def fake_corpus(n_news=20, topics=3):
    ids = torch.arange(n_news, dtype=torch.int32)
    return types.SimpleNamespace(news_category=ids % topics, news_subCategory=torch.zeros(n_news, dtype=torch.int32))


def list_args(U=3, H=6, lens=(2, 0, 3), n_news=20):
    P = sum(lens)
    return dict(news_cache=torch.zeros(n_news, 8), corpus=fake_corpus(n_news), hist_index=torch.zeros(U, H, dtype=torch.int32),
                hist_mask=torch.ones(U, H, dtype=torch.bool), user_freshness=torch.zeros(U, H), user_lifetime=torch.zeros(U, H),
                cand_offsets=torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64),
                cand_index=torch.arange(P, dtype=torch.int32), cand_freshness=torch.zeros(P), cand_lifetime=torch.zeros(P))


def test_cne_is_refused_with_score_pools_message():
    model = Model(make_config(content_encoder='CNE', **_TINY))
    a = list_args()
    shared = {k: a[k] for k in ('news_cache', 'corpus', 'hist_index', 'hist_mask', 'user_freshness', 'user_lifetime')}
    with pytest.raises(ValueError) as pool:
        model.score_pool(cand_index=torch.arange(5, dtype=torch.int32), cand_freshness=torch.zeros(5), cand_lifetime=torch.zeros(3, 5), **shared)
    for call in (lambda: model.score_lists(**list_args()), lambda: model.recommend_lists(k=2, **list_args())):
        with pytest.raises(ValueError) as lists:
            call()
        assert str(lists.value) == str(pool.value) and 'CNE' in str(lists.value)


@pytest.mark.parametrize('change,match', [
    (dict(news_cache=torch.zeros(20, 0)), 'news_cache must be'),
    (dict(news_cache=torch.zeros(20)), 'news_cache must be'),
    (dict(hist_index=torch.zeros(3, dtype=torch.int32)), r'hist_index must be \[U, H\]'),
    (dict(hist_mask=torch.ones(3, 5, dtype=torch.bool)), 'hist_mask must be'),
    (dict(user_freshness=torch.zeros(6, 3)), 'user_freshness must be'),
    (dict(user_lifetime=torch.zeros(2, 6)), 'user_lifetime must be'),
    (dict(cand_offsets=torch.tensor([0, 2, 5])), 'cand_offsets must be U \\+ 1 = 4'),
    (dict(cand_offsets=torch.tensor([1, 2, 2, 5])), 'cand_offsets must start at 0'),
    (dict(cand_offsets=torch.tensor([0, 3, 2, 5])), 'decreasing'),
    (dict(cand_offsets=torch.tensor([0, 2, 2, 4])), 'end at P = 5'),
    (dict(cand_offsets=[0.0, 2.0, 2.0, 5.0]), 'cand_offsets must be'),
    (dict(cand_index=torch.zeros(5)), 'int32 or int64'),
    (dict(cand_index=torch.zeros(1, 5, dtype=torch.int32)), r'cand_index must be \[P\]'),
    (dict(cand_freshness=torch.zeros(4)), 'cand_freshness must be'),
    (dict(cand_lifetime=torch.zeros(3, 5)), 'cand_lifetime must be'),
    (dict(pairs_per_pass=0), 'pairs_per_pass must be positive'),
])
def test_bad_arguments_are_value_errors_on_the_host(change, match):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match=match):
        model.score_lists(**dict(list_args(), **change))
    with pytest.raises(ValueError, match=match):
        model.recommend_lists(k=1, **dict(list_args(), **change))


def test_offsets_may_be_a_host_sequence():
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match='end at P = 5'):
        model.score_lists(**dict(list_args(), cand_offsets=[0, 2, 2, 4]))
    with pytest.raises(ValueError, match='end at P = 5'):
        model.score_lists(**dict(list_args(), cand_offsets=np.array([0, 2, 2, 6], dtype=np.int32)))


@pytest.mark.parametrize('k', [0, -1, 129])
def test_k_out_of_range_is_a_value_error(k):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match='1 <= k <= 128'):
        model.recommend_lists(k=k, **list_args())


def test_more_topics_than_the_plan_groups_are_refused():
    n = recommend.MAX_TOPICS + 1
    model = Model(make_config(**_TINY))
    args = dict(list_args(n_news=n), corpus=fake_corpus(n, topics=n))
    with pytest.raises(ValueError, match='8193 topics.*8192'):
        model.score_lists(**args)
    with pytest.raises(ValueError, match='8193 topics.*8192'):
        model.recommend_lists(k=3, **args)


def test_no_pairs_give_empty_results():
    model = Model(make_config(**_TINY))
    args = list_args(lens=(0, 0, 0))
    scores = model.score_lists(**args)
    assert scores.shape == (0,) and scores.dtype == torch.float32
    pos, top = model.recommend_lists(k=4, **args)
    assert pos.shape == top.shape == (3, 4) and pos.dtype == torch.int32 and top.dtype == torch.float32
    assert (pos == -1).all() and torch.isneginf(top).all()


def test_the_grouped_dev_pass_is_refused_under_cne():
    model = Model(make_config(content_encoder='CNE', **_TINY))
    with pytest.raises(ValueError, match='CNE'):
        util.evaluate_cached_on_device(model, None, [0, 0, 1], [[1, 0], [1]], grouped=True)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NEW = ('lime_list_plan_count', 'lime_list_plan', 'lime_topk_segments_workspace', 'lime_topk_segments_f32')


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
    count = lambda T, keys=one: lib.lime_list_plan_count(keys, one, 2, 5, T, one, None)
    plan = lambda T, S, order=one: lib.lime_list_plan(one, one, 2, 5, T, S, order, one, one, None)
    assert count(8, keys=None) == -1 and b'NULL' in lib.lime_last_error_string()
    assert count(0) == -1 and plan(0, 1) == -1 and plan(8, 0) == -1 and plan(8, 1, order=None) == -1
    assert count(8193) == -2 and b'8192' in lib.lime_last_error_string()
    assert plan(8193, 1) == -2 and b'8192' in lib.lime_last_error_string()
    assert lib.lime_list_plan_count(None, one, 0, 0, 8, None, None) == 0                                # no users: nothing to do
    ws = lib.lime_topk_segments_workspace
    assert ws(0, 100) == 0 and ws(3, 0) == 8 and ws(4, 4095) == 10 and ws(3, 4096) == 8 + 2 * 128 * 2
    assert ws(2, 1 << 20) == 6 + 2 * 256 * 128 * 2
    tk = lambda U, P, k, w=one, n=1 << 30: lib.lime_topk_segments_f32(one, one, U, P, k, one, one, w, n, None)
    assert tk(3, 10, 0) == -2 and tk(3, 10, 129) == -2 and b'1 <= k <= 128' in lib.lime_last_error_string()
    assert tk(-1, 10, 1) == -1 and tk(3, -1, 1) == -1
    assert tk(3, 10, 4, w=None, n=0) == -1 and b'lime_topk_segments_workspace()' in lib.lime_last_error_string()
    assert tk(3, 10, 4, n=7) == -1                                                                      # one float short
    assert tk(3, 10, 4, w=ctypes.c_void_p(20), n=8) == -1                                               # misaligned
    assert tk(0, 0, 1) == 0                                                                             # no segments: nothing to do
