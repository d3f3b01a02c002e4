"""Calibrated slates without a GPU: ``recommend.calibrated_select`` (the host statement every device test is held against) against a
literal per-round loop over the FULL KL objective; the consequences its docstring states; ``recommend.slate_miscalibration`` against a
literal statement; the share of sure rows of every shape the device tests use; the refusals of the three Model entries, of the sweep's
settings and of ``calibration=``; the ``ops`` host checks with the library out of reach; the C entries' statuses in their order."""
import ctypes
import subprocess
import types

import numpy as np
import pytest
import torch

from lime_cikm25_amd import Model, _lib, make_config, ops, recommend, util as U
from lime_cikm25_amd.build import build_library
from calibrate_cases import (GPU_SHAPES, case, check_greedy, host_select, literal_calibrated, literal_miscalibration, literal_values,
                             metric_bound, padded, sure_rows, tie_case, tolerance)
from user_cases import _TINY

LAMS = (0.0, 0.25, 0.5, 0.75, 1.0)
SMALL_SCORES = np.array([-1.0, 0.0, 1.0, 1.0, 0.25, -np.inf, np.nan, np.inf], dtype=np.float32)


def small_groups(seed=0, groups=64, rows=16):
    """``groups`` x ``rows`` (about 1,000) small cases: M <= 12, H <= 8, n_keys <= 5, k <= M, lam of five values, alpha of two; scores
    from a few values in any order (real ties), ids from -1 to n + 1 (the last two out of range), weights of {0, 0.25, 0.5, 1} in half
    of the groups, keys and history keys from -1 to n_keys (both ends out of range)."""
    rng = np.random.default_rng(seed)
    for g in range(groups):
        M, H, n_keys = int(rng.integers(1, 13)), int(rng.integers(0, 9)), int(rng.integers(1, 6))
        k = M if g % 8 == 0 else int(rng.integers(1, M + 1))
        n = int(rng.integers(1, 9))
        yield dict(scores=rng.choice(SMALL_SCORES, size=(rows, M)).astype(np.float32), ids=rng.integers(-1, n + 2, size=(rows, M)).astype(np.int32),
                   keys=rng.integers(-1, n_keys + 1, size=n).astype(np.int32), n_keys=n_keys,
                   hist_keys=rng.integers(-1, n_keys + 1, size=(rows, H)).astype(np.int32),
                   weights=rng.choice(np.array([0, 0.25, 0.5, 1.0], dtype=np.float32), size=(rows, H)) if g % 2 else None), LAMS[g % 5], (0.01, 0.1)[g % 2 ^ (g // 2) % 2], k


def test_calibrated_select_is_the_literal_loop_over_the_full_kl():
    """Every pick is a best entry of its round under the literal objective (to 1e-9: fp64 rounding is seven digits below), and the
    picks ARE the literal loop's wherever the row's gap exceeds 1e-9.  (Scores of a few exact values in any order make exact ties
    between different (group, score) classes -- 0.5 rel against 0.5 gain --, which the two fp64 evaluations break differently.)"""
    cases = moved = sure = 0
    for c, lam, alpha, k in small_groups():
        got, gap = recommend.calibrated_select(c['scores'], c['ids'], c['keys'], c['n_keys'], c['hist_keys'], c['weights'], lam, alpha, k,
                                               return_gap=True)
        R = c['scores'].shape[0]
        assert got.dtype == np.int32 and got.shape == (R, k) and gap.shape == (R,)
        plain = recommend.calibrated_select(c['scores'], c['ids'], c['keys'], c['n_keys'], c['hist_keys'], c['weights'], 1.0, alpha, k)
        for r in range(R):
            row = (c['scores'][r], c['ids'][r], c['keys'], c['n_keys'], c['hist_keys'][r], None if c['weights'] is None else c['weights'][r],
                   lam, alpha)
            taken = []
            for j in got[r]:
                values = literal_values(*row, taken)
                if j < 0:
                    assert not values, (cases, r, taken)
                    break
                assert values[int(j)] >= max(values.values()) - 1e-9, (cases, r, taken, int(j), values)
                taken.append(int(j))
            if gap[r] > 1e-9:
                sure += 1
                assert np.array_equal(got[r], padded(literal_calibrated(*row, k), k)), (cases, r, lam, alpha, k)
        cases += R
        moved += int((got != plain).any(axis=1).sum())
    assert cases >= 1000 and moved > cases // 10 and 2 * sure > cases, (cases, moved, sure)     # the gain is felt; most rows have ONE answer


def sorted_case(R, M, H, n_keys, seed, weighted=False):
    return case(R, M, H, n_keys, seed, weighted)                              # (clustered: scores descending, so rank order is score order)


@pytest.mark.parametrize('M,H', [(1, 3), (7, 6), (40, 20)])
def test_the_stated_consequences(M, H):
    c = sorted_case(6, M, H, 5, seed=M)
    live = (c['ids'] >= 0) & (c['ids'] < c['keys'].shape[0]) & np.isfinite(c['scores'])
    select = lambda lam, k, **kw: recommend.calibrated_select(c['scores'], c['ids'], c['keys'], 5, kw.get('hist', c['hist_keys']), None, lam, 0.01, k)
    for k in (1, min(M, 5), M):
        plain = select(1.0, k)                                                # lam = 1: the live entries in rank order
        blind = select(0.3, k, hist=np.full_like(c['hist_keys'], -1))         # no target: the same
        for r in range(6):
            assert np.array_equal(plain[r], padded(np.flatnonzero(live[r])[:k], k)) and np.array_equal(blind[r], plain[r])
    for lam in (0.0, 0.3, 1.0):
        every = select(lam, M)                                                # k >= the live entries: all of them, then -1
        for r in range(6):
            n_live = int(live[r].sum())
            assert sorted(every[r, :n_live].tolist()) == np.flatnonzero(live[r]).tolist() and (every[r, n_live:] == -1).all()
        for k in (1, min(M, 5)):                                              # a prefix of the picks at k is the picks at a smaller k
            assert np.array_equal(select(lam, k), every[:, :k])
    assert np.array_equal(select(0.3, min(M, 3), hist=np.zeros((6, 0), dtype=np.int32)), select(1.0, min(M, 3)))     # H = 0: no target


def test_equal_group_and_score_entries_come_out_in_rank_order():
    c = tie_case(40, 24, 10, 3, seed=5)
    for lam in (0.0, 0.4):
        picks = recommend.calibrated_select(c['scores'], c['ids'], c['keys'], 3, c['hist_keys'], None, lam, 0.01, 24)
        seen = 0
        for r in range(40):
            took = [int(j) for j in picks[r] if j >= 0]
            cls = [(int(c['keys'][c['ids'][r, j]]), float(c['scores'][r, j])) for j in took]
            for a in range(len(took)):
                for b in range(a + 1, len(took)):
                    if cls[a] == cls[b]:
                        seen += 1
                        assert took[a] < took[b], (r, took[a], took[b])
        assert seen > 100


def test_a_sport_reader_gets_a_sport_heavy_slate():
    """70 % sport and 30 % politics in the history: about seven and three of ten, where the plain slate is ten of sport."""
    keys = np.array([0] * 20 + [1] * 20, dtype=np.int32)                      # news 0-19 sport, 20-39 politics
    scores = np.r_[np.linspace(4.0, 3.0, 20), np.linspace(2.0, 1.0, 20)][None].astype(np.float32)        # sport scores high together
    ids = np.arange(40)[None]
    hist = np.array([[0] * 7 + [1] * 3])
    miss = lambda picks: recommend.slate_miscalibration(picks, 10, None, np.arange(40), keys, 2, hist)[0][0]
    plain = recommend.calibrated_select(scores, ids, keys, 2, hist, None, 1.0, 0.01, 10)
    exact = recommend.calibrated_select(scores, ids, keys, 2, hist, None, 0.0, 0.01, 10)
    mixed = recommend.calibrated_select(scores, ids, keys, 2, hist, None, 0.2, 0.01, 10)
    assert (keys[plain[0]] == 0).all() and int((keys[exact[0]] == 0).sum()) == 7 and int((keys[mixed[0]] == 0).sum()) == 9
    assert miss(exact) < 1e-12 and miss(plain) > 1.0 and miss(mixed) < miss(plain) / 5
    assert np.array_equal(np.sort(exact[0][keys[exact[0]] == 0]), np.arange(7))      # within a group the best scores are taken


def test_calibrated_select_refuses_what_it_cannot_read():
    s, i, keys, hk = np.zeros((2, 3)), np.zeros((2, 3), dtype=int), np.zeros(4, dtype=int), np.zeros((2, 5), dtype=int)
    for bad in (lambda: recommend.calibrated_select(s[0], i[0], keys, 2, hk), lambda: recommend.calibrated_select(s, i[:, :2], keys, 2, hk),
                lambda: recommend.calibrated_select(s, i, keys, 2, hk, lam=1.5), lambda: recommend.calibrated_select(s, i, keys, 2, hk, lam=float('nan')),
                lambda: recommend.calibrated_select(s, i, keys, 2, hk, alpha=0.0), lambda: recommend.calibrated_select(s, i, keys, 2, hk, alpha=1.0),
                lambda: recommend.calibrated_select(s, i, keys, 2, hk, k=0), lambda: recommend.calibrated_select(s, i, keys, 0, hk),
                lambda: recommend.calibrated_select(s, i, keys, 2, hk[0]), lambda: recommend.calibrated_select(s, i, keys, 2, hk, np.ones((2, 4)))):
        with pytest.raises(ValueError, match='calibrated_select needs'):
            bad()


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
def slate_case(seed, R=60, k=10, ldp=13, n=30, n_keys=5, H=8, lists=True, weighted=True):
    """Slates over lists (or one pool) with empty slots, positions out of range, news ids out of range, keys out of range, histories of
    which some are all masked."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 15, size=R) if lists else None
    P = int(lens.sum()) if lists else 25
    c = dict(k=k, offsets=np.r_[0, np.cumsum(lens)].astype(np.int64) if lists else None, news=rng.integers(-1, n + 2, size=P).astype(np.int32),
             keys=rng.integers(-1, n_keys + 1, size=n).astype(np.int32), n_keys=n_keys,
             positions=rng.integers(-1, 16, size=(R, ldp)).astype(np.int32), hist_keys=rng.integers(-1, n_keys, size=(R, H)).astype(np.int32),
             weights=rng.choice(np.array([0, 0.25, 0.5, 1.0, np.nan, -1.0], dtype=np.float32), size=(R, H)) if weighted else None)
    c['hist_keys'][::7] = -1                                                  # no target
    c['positions'][3::11] = -1                                                # no filled slot
    return c


def literal_slates(c, alpha):
    R = c['positions'].shape[0]
    value, status = np.zeros(R), np.zeros(R, dtype=np.int32)
    for r in range(R):
        beg, end = (0, c['news'].shape[0]) if c['offsets'] is None else (int(c['offsets'][r]), int(c['offsets'][r + 1]))
        slot_keys = []
        for pos in c['positions'][r, :c['k']]:
            if 0 <= pos < end - beg and 0 <= c['news'][beg + pos] < c['keys'].shape[0]:
                key = int(c['keys'][c['news'][beg + pos]])
                slot_keys.append(key if 0 <= key < c['n_keys'] else -1)
        hr = r % c['hist_keys'].shape[0]
        value[r], status[r] = literal_miscalibration(slot_keys, c['hist_keys'][hr], None if c['weights'] is None else c['weights'][hr], c['n_keys'], alpha)
    return value, status


@pytest.mark.parametrize('lists,weighted,alpha', [(True, True, 0.01), (False, False, 0.1), (True, False, 0.01)])
def test_slate_miscalibration_is_the_literal_statement(lists, weighted, alpha):
    c = slate_case(3, lists=lists, weighted=weighted)
    value, status = recommend.slate_miscalibration(c['positions'], c['k'], c['offsets'], c['news'], c['keys'], c['n_keys'], c['hist_keys'],
                                                   c['weights'], alpha)
    want_v, want_s = literal_slates(c, alpha)
    assert value.dtype == np.float64 and status.dtype == np.int32 and np.array_equal(status, want_s)
    assert sorted(set(status.tolist())) == [0, 1, 2] and (value[status != 0] == 0).all()
    assert np.abs(value - want_v).max() <= metric_bound(8, alpha) and value[status == 0].max() > 0.5
    lo, _ = recommend.slate_miscalibration(c['positions'], 5, c['offsets'], c['news'], c['keys'], c['n_keys'], c['hist_keys'], c['weights'], alpha)
    again, _ = recommend.slate_miscalibration(np.ascontiguousarray(c['positions'][:, :5]), 5, c['offsets'], c['news'], c['keys'], c['n_keys'],
                                              c['hist_keys'], c['weights'], alpha)
    assert np.array_equal(lo, again)                                          # a prefix is the slate at the smaller k
    hist3 = c['hist_keys'][:3]                                                # slate r reads history row r % hist_rows
    v3, _ = recommend.slate_miscalibration(c['positions'][:6], c['k'], None if c['offsets'] is None else c['offsets'][:7], c['news'], c['keys'],
                                           c['n_keys'], hist3, None, alpha)
    v6, _ = recommend.slate_miscalibration(c['positions'][:6], c['k'], None if c['offsets'] is None else c['offsets'][:7], c['news'], c['keys'],
                                           c['n_keys'], np.concatenate([hist3, hist3]), None, alpha)
    assert np.array_equal(v3, v6)


# ---- the inputs of the device tests ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', GPU_SHAPES, ids=lambda s: 'R%d-M%d-H%d-n%d-k%d-lam%g' % s[:6])
def test_the_device_shapes_hold_their_share_of_sure_rows_in_fp64_alone(shape):
    R, M, H, n_keys, k, lam, alpha, weighted, seed, share = shape
    c = case(R, M, H, n_keys, seed, weighted)
    picks, gap = host_select(c, lam, alpha, k)
    tol = tolerance(H, alpha)
    check_greedy(picks, c, lam, alpha, 1e-12, 'the statement against itself')
    if share:
        assert 4 * int(sure_rows(gap, tol).sum()) >= 3 * R, (int(sure_rows(gap, tol).sum()), R, tol)


def test_the_tolerance_is_what_the_derivation_gives():
    u = 2.0 ** -24
    assert abs(tolerance(128, 0.01) / u - 2 * (256 + 4 + 16 * (1 + 1 / (np.e * np.log(100))) + 2 * 259 / np.log(100) + 2)) < 1e-9
    assert tolerance(50, 0.01) < tolerance(128, 0.01) < 1e-4 and tolerance(6, 0.1) > tolerance(6, 0.01)
    assert 1e-14 < metric_bound(128, 0.01) < 1e-12


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def test_both_symbols_are_declared_bound_and_exported(lib):
    header = open(_lib.HEADER_PATH).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ('lime_calibrate_rows_f32', 'lime_slate_miscalibration'):
        assert name + '(' in header and name in _lib.SIGNATURES and getattr(lib, name) is not None and ' T %s\n' % name in exported
    assert _lib.ABI_VERSION == 14 and lib.lime_abi_version() == 14            # an added entry leaves the version alone


def test_the_selection_entry_refuses_in_its_documented_order_without_a_launch(lib):
    one = ctypes.c_void_p(16)                       # a non-NULL, 16-byte aligned address: never dereferenced by a refused call
    BAD_ARG, UNSUPPORTED = _lib.CONSTANTS['LIME_ERR_BAD_ARG'], _lib.CONSTANTS['LIME_ERR_UNSUPPORTED']

    def cal(scores=one, ids=one, R=3, M=16, keys=one, n=5, n_keys=4, hist_keys=one, hist_weight=one, hist_rows=3, H=6, lam=0.5, alpha=0.01, k=4,
            picks=one):
        return lib.lime_calibrate_rows_f32(scores, ids, R, M, keys, n, n_keys, hist_keys, hist_weight, hist_rows, H, lam, alpha, k, picks, None)
    # 1. a NULL pointer, ahead of everything else
    for name in ('scores', 'ids', 'keys', 'hist_keys', 'picks'):
        assert cal(**{name: None}, M=0, H=200) == BAD_ARG and b'NULL' in lib.lime_last_error_string()
    # 2. the dimensions, then lam, then alpha, ahead of the limits
    for bad in (dict(R=-1), dict(M=0, k=0), dict(k=0), dict(k=17), dict(n=0), dict(n_keys=0), dict(H=-1), dict(hist_rows=0), dict(hist_rows=-1, H=0)):
        assert cal(**bad) == BAD_ARG and b'bad dims' in lib.lime_last_error_string(), bad
        assert cal(**{'H': 200, **bad}) == BAD_ARG, bad                # (with something unsupported beside it)
    for bad in (-0.01, 1.01, float('nan'), float('inf')):
        assert cal(lam=bad, alpha=2.0, H=200) == BAD_ARG and b'lam' in lib.lime_last_error_string()
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan')):
        assert cal(alpha=bad, H=200) == BAD_ARG and b'alpha' in lib.lime_last_error_string()
    # 3. the limits
    assert cal(M=129) == UNSUPPORTED and b'128' in lib.lime_last_error_string()
    assert cal(H=129) == UNSUPPORTED and cal(n_keys=8193) == UNSUPPORTED and cal(n_keys=8192, R=0) == 0
    # no rows: a success without a launch, whatever the pointers hold -- but after the checks
    assert cal(R=0) == 0 and cal(R=0, M=128, k=128, H=128, lam=0.0) == 0 and cal(R=0, hist_weight=None) == 0 and cal(R=0, H=0, hist_rows=0) == 0
    assert cal(R=0, k=17) == BAD_ARG and cal(R=0, H=129) == UNSUPPORTED


def test_the_metric_entry_refuses_in_its_documented_order_without_a_launch(lib):
    one = ctypes.c_void_p(16)
    BAD_ARG, UNSUPPORTED = _lib.CONSTANTS['LIME_ERR_BAD_ARG'], _lib.CONSTANTS['LIME_ERR_UNSUPPORTED']

    def mis(positions=one, R=3, ldp=12, k=10, offsets=one, news=one, P=20, keys=one, n=5, n_keys=4, hist_keys=one, hist_weight=one, hist_rows=3,
            H=6, alpha=0.01, value=one, status=one):
        return lib.lime_slate_miscalibration(positions, R, ldp, k, offsets, news, P, keys, n, n_keys, hist_keys, hist_weight, hist_rows, H, alpha,
                                             value, status, None)
    for name in ('positions', 'news', 'keys', 'hist_keys', 'value', 'status'):
        assert mis(**{name: None}, k=0, H=200) == BAD_ARG and b'NULL' in lib.lime_last_error_string()
    for bad in (dict(R=-1), dict(P=-1), dict(k=0), dict(k=13), dict(n=0), dict(n_keys=0), dict(H=-1), dict(hist_rows=0)):
        assert mis(**bad) == BAD_ARG and b'bad dims' in lib.lime_last_error_string(), bad
        assert mis(**{'H': 200, **bad}) == BAD_ARG or 'H' in bad, bad
    for bad in (0.0, 1.0, float('nan')):
        assert mis(alpha=bad, H=200) == BAD_ARG and b'alpha' in lib.lime_last_error_string()
    assert mis(k=129, ldp=200) == UNSUPPORTED and mis(H=129) == UNSUPPORTED and mis(n_keys=8193) == UNSUPPORTED
    assert mis(R=0) == 0 and mis(R=0, offsets=None, hist_weight=None) == 0 and mis(R=0, k=128, ldp=128, H=128) == 0
    assert mis(R=0, k=13) == BAD_ARG and mis(R=0, k=129, ldp=200) == UNSUPPORTED


# ---- ops: the host checks, with the library out of reach --------------------------------------------------------------------------------
def no_library():
    raise AssertionError('the library was reached: a launch would follow')


def test_ops_refuse_without_a_launch(monkeypatch):
    monkeypatch.setattr(_lib, 'load', no_library)
    s, i, keys, hk = torch.zeros((2, 4)), torch.zeros((2, 4), dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.calibrate_rows(s, i, keys, 3, hk, None, 0.5, 0.01, 2)             # CPU tensors: the HIP path has no CPU fallback
    with pytest.raises(TypeError):
        ops.slate_miscalibration(i, 2, None, keys, keys, 3, hk)
    if torch.cuda.is_available():
        s, i, keys, hk = s.cuda(), i.cuda(), keys.cuda(), hk.cuda()
        for bad in (dict(k=5), dict(k=0), dict(lam=1.5), dict(lam=float('nan')), dict(alpha=0.0), dict(alpha=1.0), dict(n_keys=0), dict(n_keys=8193)):
            with pytest.raises(ValueError, match='calibrate_rows needs'):
                ops.calibrate_rows(s, i, keys, **{'n_keys': 3, 'hist_keys': hk, 'hist_weight': None, 'lam': 0.5, 'alpha': 0.01, 'k': 2, **bad})
        with pytest.raises(ValueError, match='contiguous'):
            ops.calibrate_rows(torch.zeros((2, 8)).cuda()[:, :4], i, keys, 3, hk, None, 0.5, 0.01, 2)
        with pytest.raises(TypeError):
            ops.calibrate_rows(s, i.long(), keys, 3, hk, None, 0.5, 0.01, 2)
        with pytest.raises(ValueError):
            ops.calibrate_rows(s, i[:1], keys, 3, hk, None, 0.5, 0.01, 2)
        with pytest.raises(TypeError):
            ops.calibrate_rows(s, i, keys.long(), 3, hk, None, 0.5, 0.01, 2)
        with pytest.raises(TypeError):
            ops.calibrate_rows(s, i, keys, 3, hk.long(), None, 0.5, 0.01, 2)
        with pytest.raises(ValueError, match='H <= 128'):
            ops.calibrate_rows(s, i, keys, 3, torch.zeros((2, 129), dtype=torch.int32).cuda(), None, 0.5, 0.01, 2)
        with pytest.raises(ValueError, match='hist_rows >= 1'):
            ops.calibrate_rows(s, i, keys, 3, hk[:0], None, 0.5, 0.01, 2)
        with pytest.raises(ValueError, match='hist_weight'):
            ops.calibrate_rows(s, i, keys, 3, hk, torch.zeros((2, 4)).cuda(), 0.5, 0.01, 2)
        with pytest.raises(TypeError):
            ops.calibrate_rows(s, i, keys, 3, hk, torch.zeros((2, 3), dtype=torch.float64).cuda(), 0.5, 0.01, 2)
        assert ops.calibrate_rows(s[:0], i[:0], keys, 3, hk, None, 0.5, 0.01, 2).shape == (0, 2)        # no rows: no call
        off = torch.tensor([0, 2, 5]).cuda()
        for bad in (dict(k=5), dict(k=0), dict(alpha=0.0), dict(n_keys=8193)):
            with pytest.raises(ValueError, match='slate_miscalibration needs'):
                ops.slate_miscalibration(i, **{'k': 2, 'offsets': off, 'news': keys, 'keys': keys, 'n_keys': 3, 'hist_keys': hk, **bad})
        with pytest.raises(ValueError):
            ops.slate_miscalibration(i, 2, off[:2], keys, keys, 3, hk)         # offsets: R + 1 entries
        with pytest.raises(TypeError):
            ops.slate_miscalibration(i, 2, off.int(), keys, keys, 3, hk)
        with pytest.raises(TypeError):
            ops.slate_miscalibration(i.long(), 2, off, keys, keys, 3, hk)
        with pytest.raises(TypeError):
            ops.slate_miscalibration(i, 2, off, keys, keys, 3, hk.cpu())
        value, status = ops.slate_miscalibration(i[:0], 2, off[:1], keys, keys, 3, hk)
        assert value.shape == (0,) and value.dtype == torch.float64 and status.dtype == torch.int32


# ---- the Model entries ---------------------------------------------------------------------------------------------------------------
def a_corpus(n_news=20, groups=4):
    return types.SimpleNamespace(news_category=torch.arange(n_news) % groups, news_subCategory=torch.zeros(n_news, dtype=torch.long))


def users(U=3, H=6, n_news=20, corpus=None):
    return dict(news_cache=torch.zeros(n_news, 8), corpus=corpus, hist_index=torch.zeros(U, H, dtype=torch.int32),
                hist_mask=torch.ones(U, H, dtype=torch.bool), user_freshness=torch.zeros(U, H), user_lifetime=torch.zeros(U, H))


def entries(model, U=3, C=5, H=6, n_news=20, corpus=None, **more):
    pool = dict(users(U, H, n_news, corpus), cand_index=torch.arange(C, dtype=torch.int32), cand_freshness=torch.zeros(C),
                cand_lifetime=torch.zeros(U, C), k=2)
    lists = dict(users(U, H, n_news, corpus), cand_offsets=torch.tensor([0, 2, 2, C]), cand_index=torch.arange(C, dtype=torch.int32),
                 cand_freshness=torch.zeros(C), cand_lifetime=torch.zeros(C), k=2)
    return [lambda **kw: model.recommend(**{**pool, **more, **kw}),
            lambda **kw: model.recommend_schedule(slot_offsets=torch.zeros(2), **{**pool, **more, **kw}),
            lambda **kw: model.recommend_lists(**{**lists, **more, **kw})]


@pytest.fixture(scope='module')
def model():
    return Model(make_config(**_TINY))                                         # never moved to a device: a refusal precedes any launch


@pytest.mark.parametrize('bad', [-0.1, 1.5, float('nan'), '0.5', True, 1 + 0j])
def test_calibrate_lambda_must_be_a_real_in_the_unit_interval(model, bad):
    for entry in entries(model):                                              # (corpus=None: nothing reads the corpus before this)
        with pytest.raises(ValueError, match=r'calibrate_lambda must be a real number in \[0, 1\]'):
            entry(calibrate_lambda=bad)


def test_the_scalar_refusals_come_before_the_corpus(model):
    for entry in entries(model):
        for bad in ('subtopic', None, 3):
            with pytest.raises(ValueError, match="calibrate_by must be 'category' or 'topic'"):
                entry(calibrate_lambda=0.5, calibrate_by=bad)
        for bad in (0.0, 1.0, -0.1, float('nan'), '0.01', True, None):
            with pytest.raises(ValueError, match=r'calibrate_alpha must be a real number in \(0, 1\)'):
                entry(calibrate_lambda=0.5, calibrate_alpha=bad)
        for bad in (np.ones((3, 6), dtype=np.float32), torch.ones(3, 6, dtype=torch.float64), torch.ones(18), [[1.0] * 6] * 3):
            with pytest.raises(ValueError, match=r'calibrate_weights must be an fp32 tensor \[U, H\]'):
                entry(calibrate_lambda=0.5, calibrate_weights=bad)
        for bad in (1, 129, 64.0, True):
            with pytest.raises(ValueError, match=r'shortlist must be an integer in \[k, 128\] = \[2, 128\]'):
                entry(calibrate_lambda=0.5, shortlist=bad)
        with pytest.raises(ValueError, match='together with mmr_lambda is out of scope'):
            entry(calibrate_lambda=0.5, mmr_lambda=0.5)
        for alone in (dict(calibrate_by='topic'), dict(calibrate_alpha=0.1), dict(calibrate_weights=torch.ones(3, 6))):
            with pytest.raises(ValueError, match='are read with calibrate_lambda alone'):
                entry(**alone)


def test_the_refusals_that_read_the_corpus_and_the_histories(model):
    for entry in entries(model, corpus=a_corpus()):
        for bad in (torch.ones(3, 5), torch.ones(2, 6), torch.ones(3, 6, device='meta')):
            with pytest.raises(ValueError, match=r'calibrate_weights must be fp32 \[U, H\] = \[3, 6\]'):
                entry(calibrate_lambda=0.5, calibrate_weights=bad)
        with pytest.raises(ValueError, match='pairs_per_pass must be positive'):          # valid arguments refuse nothing themselves
            entry(pairs_per_pass=0, calibrate_lambda=0.5, calibrate_by='topic', calibrate_alpha=0.1, calibrate_weights=torch.ones(3, 6), shortlist=2)
        with pytest.raises(ValueError, match='keeps 1 <= k <= 128'):                      # a bad k stays the entry's own refusal
            entry(k=0, calibrate_lambda=0.5)
    for entry in entries(model, n_news=9000, corpus=a_corpus(9000, 9000)):
        with pytest.raises(ValueError, match='the corpus has 9000 groups by category, lime_calibrate_rows_f32 counts up to 8192'):
            entry(calibrate_lambda=0.5)
    for entry in entries(model, H=129, corpus=a_corpus()):
        with pytest.raises(ValueError, match='reads up to 128 history slots'):
            entry(calibrate_lambda=0.5)


def test_shortlist_and_similarity_without_a_lambda_keep_their_words(model):
    for entry in entries(model):
        with pytest.raises(ValueError, match='shortlist and similarity are read with mmr_lambda alone: give mmr_lambda, or neither of them'):
            entry(shortlist=64)
        with pytest.raises(ValueError, match='shortlist and similarity are read with mmr_lambda alone: give mmr_lambda, or neither of them'):
            entry(similarity=torch.zeros(20, 8))
    for entry in entries(model, corpus=a_corpus()):
        with pytest.raises(ValueError, match='shortlist and similarity are read with mmr_lambda alone'):
            entry(calibrate_lambda=0.5, similarity=torch.zeros(20, 8))           # the similarity is MMR's alone


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
def fake_split(H=4):
    corpus = types.SimpleNamespace(news_category=torch.tensor([0, 1, 1, 2, 2]), news_subCategory=torch.tensor([0, 3, 4, 3, 3]))
    model = types.SimpleNamespace(reads_content_mask=False, build_news_cache=lambda corpus: no_library())
    return model, types.SimpleNamespace(corpus=corpus, num=3, hist_index=torch.zeros(3, H, dtype=torch.int32))


@pytest.mark.parametrize('settings,calibration,H,match', [
    ([{'calibrate_lambda': 1.5}], None, 4, 'calibrate_lambda'),
    ([{}, {'calibrate_lambda': 0.5, 'calibrate_by': 'user'}], None, 4, 'calibrate_by'),
    ([{'calibrate_lambda': 0.5, 'calibrate_alpha': 1.0}], None, 4, 'calibrate_alpha'),
    ([{'calibrate_alpha': 0.1}], None, 4, 'calibrate_lambda alone'),
    ([{'calibrate_by': 'topic'}], None, 4, 'calibrate_lambda alone'),
    ([{'calibrate_lambda': 0.5, 'mmr_lambda': 0.5}], None, 4, 'out of scope'),
    ([{'calibrate_lambda': 0.5, 'shortlist': 3}], None, 4, 'shortlist'),
    ([{'shortlist': 64}], None, 4, 'mmr_lambda alone'),
    ([{'calibrate_lambda': 0.5}], None, 129, '128 history slots'),
    ([{'calibrate_weights': None}], None, 4, 'unknown key'),
    ([{}], 'user', 4, 'calibration must be'),
    ([{}], 'category', 129, '128 history slots'),
    ([{}], True, 4, 'calibration must be'),
])
def test_evaluate_slates_refuses_a_bad_calibration_before_any_scoring(monkeypatch, settings, calibration, H, match):
    monkeypatch.setattr(_lib, 'load', no_library)
    model, behaviors = fake_split(H)
    with pytest.raises(ValueError, match=match):
        U.evaluate_slates_on_device(model, behaviors, [0, 0, 1], [[1, 0], [1]], settings, k=5, calibration=calibration)


def test_the_setting_keys_and_the_trainer_pass_calibration_through(monkeypatch):
    from lime_cikm25_amd.trainer import Trainer
    assert {'calibrate_lambda', 'calibrate_by', 'calibrate_alpha'} <= set(U.SLATE_SETTING_KEYS)
    assert U.SLATE_RESULT_KEYS == ('ndcg', 'rr', 'hit', 'recall', 'ild', 'topics', 'filled', 'value')
    model, behaviors = fake_split()
    checked = U.check_slate_settings(model, behaviors.corpus, [{}, {'calibrate_lambda': 0.25, 'calibrate_by': 'topic', 'shortlist': 7}], 5,
                                     calibration='category', H=4)
    assert checked[0][4] is None and checked[1][1] is None
    cal = checked[1][4]
    assert (cal.lam, cal.shortlist, cal.by, cal.alpha, cal.n_keys) == (0.25, 7, 'topic', recommend.CALIBRATE_ALPHA, 4)
    assert cal.topic_of_news.tolist() == [0, 1, 2, 3, 3]
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(ValueError, match='slate_eval must be'):
        Trainer(None, None, None, device_eval=True, slate_eval=dict(settings=[{}], calibrate='category'))
    with pytest.raises(ValueError, match='device_eval'):
        Trainer(None, None, None, slate_eval=dict(settings=[{}], k=5, calibration='category'))
