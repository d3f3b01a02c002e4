"""Diverse slates without a GPU: ``recommend.mmr_select`` (the host statement that every device test is held against) against a
literal per-round loop on exact cases with real ties; the three consequences its docstring states; a hand-made slate of duplicates; the
C entry's refusals in their documented order; the Python-level refusals of the three Model entries."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from lime_cikm25_amd import Model, _lib, make_config, recommend
from lime_cikm25_amd.build import build_library
from mmr_cases import clustered, exact_groups, literal_mmr, padded
from user_cases import _TINY


def test_mmr_select_is_the_literal_loop_on_exact_cases_with_ties():
    cases = ties = 0
    for scores, ids, table, lam, k in exact_groups():
        got, gap = recommend.mmr_select(scores, ids, table, lam, k, return_gap=True)
        assert got.dtype == np.int32 and got.shape == (scores.shape[0], k) and gap.shape == (scores.shape[0],)
        for r in range(scores.shape[0]):
            assert np.array_equal(got[r], padded(literal_mmr(scores[r], ids[r], table, lam, k), k)), (cases, r, lam, k)
        cases += scores.shape[0]
        ties += int((gap == 0).sum())
    assert cases >= 1000 and ties > cases // 4                                # the tie rule is felt


def test_dead_entries_are_never_taken_and_never_read():
    table = np.full((3, 4), np.nan, dtype=np.float32)                         # rows 1 and 2 belong to dead entries only
    table[0] = [1, 0, 0, 0]
    scores = np.array([[np.nan, 3, 2, -np.inf, 1, np.inf]], dtype=np.float32)
    ids = np.array([[1, 0, 7, 2, -1, 2]])
    assert recommend.mmr_select(scores, ids, table, 0.5, 3).tolist() == [[1, -1, -1]]
    assert recommend.mmr_select(scores[:, :1], ids[:, :1], table, 0.5, 1).tolist() == [[-1]]


@pytest.mark.parametrize('M,E', [(1, 4), (7, 8), (40, 20)])
def test_the_three_consequences(M, E):
    scores, ids, table = clustered(6, M, E, seed=M)
    live = (ids >= 0) & (ids < table.shape[0]) & np.isfinite(scores)
    for k in (1, min(M, 5), M):
        plain = recommend.mmr_select(scores, ids, table, 1.0, k)              # lam = 1: the live entries in rank order
        greedy = recommend.mmr_select(scores, ids, table, 0.0, k)             # lam = 0: `first` first
        for r in range(scores.shape[0]):
            ranks = np.flatnonzero(live[r])
            assert np.array_equal(plain[r], padded(ranks[:k], k))
            assert greedy[r, 0] == (ranks[0] if ranks.size else -1)
    for lam in (0.0, 0.3, 1.0):                                               # k >= the live entries: all of them, then -1
        every = recommend.mmr_select(scores, ids, table, lam, M)
        for r in range(scores.shape[0]):
            n_live = int(live[r].sum())
            assert sorted(every[r, :n_live].tolist()) == np.flatnonzero(live[r]).tolist() and (every[r, n_live:] == -1).all()


def test_one_duplicate_makes_room_for_the_third_story():
    table = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], dtype=np.float32)      # news 0 and 1 tell one event
    scores, ids = np.array([[3.0, 2.9, 1.0]], dtype=np.float32), np.array([[0, 1, 2]])
    assert recommend.mmr_select(scores, ids, table, 1.0, 2).tolist() == [[0, 1]]         # the plain top 2: both duplicates
    assert recommend.mmr_select(scores, ids, table, 0.5, 2).tolist() == [[0, 2]]         # 0.5 * 0.95 - 0.5 * 1 < 0.5 * 0 - 0
    picks, gap = recommend.mmr_select(scores, ids, table, 0.5, 2, return_gap=True)
    assert picks.tolist() == [[0, 2]] and abs(gap[0] - 0.025) < 1e-6            # round 1: 0.5 against 0.475; round 2: 0 against -0.025


def test_mmr_select_refuses_what_it_cannot_read():
    s, i, t = np.zeros((2, 3)), np.zeros((2, 3), dtype=int), np.ones((4, 4))
    for bad in (lambda: recommend.mmr_select(s[0], i[0], t, 0.5, 1), lambda: recommend.mmr_select(s, i[:, :2], t, 0.5, 1),
                lambda: recommend.mmr_select(s, i, t, 1.5, 1), lambda: recommend.mmr_select(s, i, t, float('nan'), 1),
                lambda: recommend.mmr_select(s, i, t, 0.5, 0)):
        with pytest.raises(ValueError, match='mmr_select needs'):
            bad()


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def test_the_new_symbol_is_declared_bound_and_exported(lib):
    header = open(_lib.HEADER_PATH).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert 'lime_mmr_rows_f32(' in header and 'lime_mmr_rows_f32' in _lib.SIGNATURES and lib.lime_mmr_rows_f32 is not None
    assert ' T lime_mmr_rows_f32\n' in exported


def test_the_entry_refuses_in_its_documented_order_without_a_launch(lib):
    one = ctypes.c_void_p(16)                       # a non-NULL, 16-byte aligned address: never dereferenced by a refused call
    BAD_ARG, UNSUPPORTED = _lib.CONSTANTS['LIME_ERR_BAD_ARG'], _lib.CONSTANTS['LIME_ERR_UNSUPPORTED']

    def mmr(scores=one, ids=one, R=3, M=16, table=one, ld=8, n=5, E=8, lam=0.5, k=4, picks=one):
        return lib.lime_mmr_rows_f32(scores, ids, R, M, table, ld, n, E, lam, k, picks, None)
    # 1. a NULL pointer, ahead of everything else
    for name in ('scores', 'ids', 'table', 'picks'):
        assert mmr(**{name: None}, M=0, E=6) == BAD_ARG and b'NULL' in lib.lime_last_error_string()
    # 2. the dimensions and lam, ahead of the limits
    for bad in (dict(R=-1), dict(M=0, k=0), dict(k=0), dict(k=17), dict(n=0), dict(E=0, ld=0), dict(ld=7), dict(lam=-0.01), dict(lam=1.01),
                dict(lam=float('nan')), dict(lam=float('inf'))):
        assert mmr(**bad) == BAD_ARG, bad
        assert mmr(**{'R': 70000, **bad}) == BAD_ARG, bad                    # (with something unsupported beside it)
    assert mmr(M=200, k=201, E=6, R=70000) == BAD_ARG and mmr(M=200, k=4, E=6, R=70000, lam=2.0) == BAD_ARG
    assert mmr(lam=2.0) == BAD_ARG and b'lam' in lib.lime_last_error_string()
    # 3. the limits
    assert mmr(M=129, k=4) == UNSUPPORTED and b'128' in lib.lime_last_error_string()
    assert mmr(E=6) == UNSUPPORTED and mmr(E=10, ld=12) == UNSUPPORTED and mmr(R=65536) == UNSUPPORTED
    # no rows: a success without a launch, whatever the pointers hold -- but after the checks
    assert mmr(R=0) == 0 and mmr(R=0, M=128, k=128, lam=0.0) == 0 and mmr(R=0, lam=1.0) == 0
    assert mmr(R=0, k=17) == BAD_ARG and mmr(R=0, E=6) == UNSUPPORTED


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


@pytest.fixture(scope='module')
def model():
    return Model(make_config(**_TINY))                                         # never moved to a device: a refusal precedes any launch


@pytest.mark.parametrize('bad', [-0.1, 1.5, float('nan'), '0.5', True, 1 + 0j])
def test_mmr_lambda_must_be_a_real_in_the_unit_interval(model, bad):
    for entry in entries(model):
        with pytest.raises(ValueError, match=r'mmr_lambda must be a real number in \[0, 1\]'):
            entry(mmr_lambda=bad)


@pytest.mark.parametrize('bad', [1, 129, 0, 64.0, '64', True])
def test_shortlist_must_be_an_integer_from_k_to_128(model, bad):
    for entry in entries(model):
        with pytest.raises(ValueError, match=r'shortlist must be an integer in \[k, 128\] = \[2, 128\]'):
            entry(mmr_lambda=0.5, shortlist=bad)


def test_similarity_must_be_an_fp32_table_over_the_cache_rows(model):
    for entry in entries(model):
        for bad in (torch.zeros(19, 8), torch.zeros(20, 8, dtype=torch.float64), torch.zeros(20), torch.zeros(20, 8, device='meta'),
                    torch.zeros(20, 6), np.zeros((20, 8), dtype=np.float32)):
            with pytest.raises(ValueError, match=r'similarity must be fp32 \[n_news, E\] = \[20, E\]'):
                entry(mmr_lambda=0.5, similarity=bad)


def test_shortlist_and_similarity_belong_to_mmr_lambda(model):
    for entry in entries(model):
        with pytest.raises(ValueError, match='shortlist and similarity are read with mmr_lambda alone'):
            entry(shortlist=64)
        with pytest.raises(ValueError, match='shortlist and similarity are read with mmr_lambda alone'):
            entry(similarity=torch.zeros(20, 8))


def test_without_mmr_the_old_refusals_are_what_they_were(model):
    for entry in entries(model):
        with pytest.raises(ValueError, match='pairs_per_pass must be positive'):
            entry(pairs_per_pass=0)
        with pytest.raises(ValueError, match='pairs_per_pass must be positive'):          # valid MMR arguments refuse nothing themselves
            entry(pairs_per_pass=0, mmr_lambda=0.5, shortlist=2, similarity=torch.zeros(20, 12))
        with pytest.raises(ValueError, match='keeps 1 <= k <= 128'):                      # a bad k stays the entry's own refusal
            entry(k=0, mmr_lambda=0.5)
