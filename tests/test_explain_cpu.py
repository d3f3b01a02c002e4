"""Explanations without a GPU: ``recommend.explain_pairs`` -- the host statement of lime_grouped_match_explain_f32 that the GPU tests
compare with -- on hand-made operands, the entry's place in the header, the derived binding and the export table, what the entry
refuses before any launch, and the host refusals of Model.explain_lists / Model.explain."""
import ctypes
import subprocess
import types

import numpy as np
import pytest
import torch

from lime_cikm25_amd import Model, make_config, recommend, _lib
from lime_cikm25_amd.build import build_library

from user_cases import _TINY

H, A, D = 5, 4, 8
SIZES = [3, 0, 4]                     # pairs per group; the middle group is empty


def operands(seed=0):
    """Three groups of H slots; group 2 has two identical history rows (slots 0 and 1): their terms tie."""
    rng = np.random.default_rng(seed)
    G, P = len(SIZES), sum(SIZES)
    kp, g = rng.normal(size=(G * H, A)), rng.normal(size=(G * H, D))
    kp[2 * H + 1], g[2 * H + 1] = kp[2 * H], g[2 * H]
    return dict(kp=kp, g=g, qp=rng.normal(size=(P, A)), cand=rng.normal(size=(P, D)), remaining=rng.uniform(-3, 3, size=P),
                offsets=np.concatenate([[0], np.cumsum(SIZES)]), H=H, scale=0.5)


def explain(d, **kw):
    kw = dict(dict(alpha=0.7, beta=0.3, use_weight=True, use_penalty=True, m=3), **kw)
    return recommend.explain_pairs(d['kp'], d['g'], d['qp'], d['cand'], d['remaining'], d['offsets'], d['H'], d['scale'], **kw)


@pytest.mark.parametrize('use_weight,use_penalty', [(False, False), (True, False), (True, True)])
def test_attention_sums_to_one_and_contributions_to_the_logit(use_weight, use_penalty):
    d = operands()
    r = explain(d, use_weight=use_weight, use_penalty=use_penalty)
    assert np.abs(r.attn.sum(axis=1) - 1.0).max() < 1e-14
    assert np.abs(r.contrib.sum(axis=1) - r.logits).max() < 1e-14
    assert np.allclose(r.logits, r.base * r.weight, rtol=0, atol=1e-15)
    if not use_weight:
        assert (r.weight == 1.0).all()
    else:
        rem = d['remaining']
        sig = 1.0 / (1.0 + np.exp(-0.7 * (rem if use_penalty else np.abs(rem))))
        assert np.allclose(r.weight, np.where((rem < 0) & use_penalty, 0.3 * sig, sig), rtol=1e-15)
    # the same numbers, written out pair by pair
    for i in range(len(SIZES)):
        for p in range(d['offsets'][i], d['offsets'][i + 1]):
            s = d['kp'][i * H:(i + 1) * H] @ d['qp'][p] * d['scale']
            a = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
            assert np.allclose(r.attn[p], a, rtol=1e-13)
            assert np.allclose(r.contrib[p], a * (d['g'][i * H:(i + 1) * H] @ d['cand'][p]) * r.weight[p], rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('by', ['contribution', 'attention'])
def test_masked_out_slots_are_never_selected_and_the_softmax_stays_unmasked(by):
    d = operands(1)
    mask = np.ones((3, H), dtype=bool)
    mask[0, [1, 4]] = False
    mask[2, 0] = False
    r, free = explain(d, mask=mask, by=by, m=3), explain(d, by=by, m=3)
    assert np.array_equal(r.attn, free.attn) and np.array_equal(r.contrib, free.contrib) and np.array_equal(r.logits, free.logits)
    values = r.contrib if by == 'contribution' else r.attn
    for p in range(sum(SIZES)):
        i = 0 if p < 3 else 2
        open_slots = np.flatnonzero(mask[i])
        assert set(r.top_slot[p].tolist()) <= set(open_slots.tolist())
        want = open_slots[np.argsort(-values[p, open_slots], kind='stable')][:3]
        assert r.top_slot[p].tolist() == want.tolist()
        assert np.array_equal(r.top_value[p], values[p, want])
        assert (np.diff(r.top_value[p]) <= 0).all()


def test_a_duplicated_history_row_ties_and_the_lower_slot_comes_first():
    d = operands(2)
    r = explain(d, m=H)
    for p in range(3, 7):                                                  # group 2: slots 0 and 1 are the same row
        assert r.contrib[p, 0] == r.contrib[p, 1] and r.attn[p, 0] == r.attn[p, 1]
        at = r.top_slot[p].tolist()
        assert at.index(1) == at.index(0) + 1
    by_attention = explain(d, m=H, by='attention')
    for p in range(3, 7):
        at = by_attention.top_slot[p].tolist()
        assert at.index(1) == at.index(0) + 1


def test_fewer_eligible_slots_than_top_pad_and_an_all_masked_row_names_nothing():
    d = operands(3)
    mask = np.zeros((3, H), dtype=bool)
    mask[0, [2, 4]] = True                                                 # two eligible slots; group 2's row is all zero
    r = explain(d, mask=mask, m=4)
    for p in range(3):
        assert sorted(r.top_slot[p, :2].tolist()) == [2, 4] and r.top_slot[p, 2:].tolist() == [-1, -1]
        assert (r.top_value[p, 2:] == 0).all() and r.top_value[p, 0] >= r.top_value[p, 1]
    assert (r.top_slot[3:] == -1).all() and (r.top_value[3:] == 0).all()
    assert np.isfinite(r.logits).all() and np.abs(r.contrib.sum(axis=1) - r.logits).max() < 1e-14


def test_a_shared_mask_row_is_read_through_hist_div():
    d = operands(4)
    d['offsets'] = np.array([0, 3, 5, 7])                                  # three groups, the first two share mask row 0
    mask = np.zeros((2, H), dtype=bool)
    mask[0, 3] = True
    mask[1, 1] = True
    r = explain(d, mask=mask, hist_div=2, m=1)
    assert r.top_slot[:5, 0].tolist() == [3] * 5 and r.top_slot[5:, 0].tolist() == [1, 1]


def test_the_indexed_and_the_composed_forms_are_the_plain_form_on_the_gathered_rows():
    d = operands(5)
    rng = np.random.default_rng(6)
    P = sum(SIZES)
    qa, ca, qt, ct = rng.normal(size=(9, A)), rng.normal(size=(9, D)), rng.normal(size=(4, A)), rng.normal(size=(4, D))
    index, occ = rng.integers(0, 9, size=P), rng.integers(0, 4, size=P)
    plain = explain(dict(d, qp=qa[index], cand=ca[index]))
    indexed = explain(dict(d, qp=qa, cand=ca), index=index)
    assert all(np.array_equal(a, b) for a, b in zip(plain, indexed))
    composed = explain(dict(d, qp=qa, cand=ca), index=index, occ=occ, qt=qt, ct=ct)
    summed = explain(dict(d, qp=qa[index] + qt[occ], cand=ca[index] + ct[occ]))
    assert all(np.array_equal(a, b) for a, b in zip(composed, summed))
    wild = explain(dict(d, qp=qa, cand=ca), index=np.where(np.arange(P) % 2, index, 100), occ=np.where(np.arange(P) % 3, occ, -7), qt=qt, ct=ct)
    clamped = explain(dict(d, qp=qa, cand=ca), index=np.where(np.arange(P) % 2, index, 8), occ=np.where(np.arange(P) % 3, occ, 0), qt=qt, ct=ct)
    assert all(np.array_equal(a, b) for a, b in zip(wild, clamped))


def test_top_slots_orders_zeros_and_nans_as_the_device_keys_do():
    v = np.array([[0.0, -0.0, np.nan, 1.0, -np.inf, 1.0]], dtype=np.float32)
    slot, top = recommend.top_slots(v, np.ones_like(v, dtype=bool), 6)
    assert slot.tolist() == [[3, 5, 0, 1, 4, 2]]
    assert top.dtype == np.float32 and np.signbit(top[0, 3]) and np.isnan(top[0, 5])


@pytest.mark.parametrize('kw', [dict(m=0), dict(m=6), dict(m=17), dict(by='gradient'), dict(hist_div=0),
                                dict(index=np.zeros(7, dtype=np.int64), occ=np.zeros(7, dtype=np.int64))])
def test_the_host_statement_refuses_what_the_entry_refuses(kw):
    with pytest.raises(ValueError):
        explain(operands(), **kw)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
NAME = 'lime_grouped_match_explain_f32'


@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def test_the_entry_is_declared_bound_and_exported(lib):
    header = open(_lib.HEADER_PATH).read()
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert NAME + '(' in header and (' T ' + NAME + '\n') in exported
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int32 and len(args) == 34 and getattr(lib, NAME) is not None
    assert args[9] is ctypes.c_int64 and args[11] is ctypes.c_int64                                 # n, n_occ
    assert args[13:16] == [ctypes.c_int32] * 3                                                      # hist_div, m, by
    assert args[23:25] == [ctypes.c_int64] * 2 and args[28:31] == [ctypes.c_float] * 3              # G, P; scale, alpha_s, beta_s
    assert _lib.CONSTANTS['LIME_EXPLAIN_BY_CONTRIBUTION'] == 0 and _lib.CONSTANTS['LIME_EXPLAIN_BY_ATTENTION'] == 1
    assert lib.lime_abi_version() == _lib.ABI_VERSION == 14                                         # an addition: no existing signature moved


def test_the_entry_refuses_bad_arguments_without_a_launch(lib):
    one = ctypes.c_void_p(16)                       # a non-NULL, 16-byte aligned address: never dereferenced by a refused call
    base = dict(kp=one, g=one, qp=one, cand=one, qt=None, ct=None, remaining=None, offsets=one, index=None, n=0, occ=None, n_occ=0, mask=one,
                hist_div=1, m=3, by=0, logits=one, base=one, weight=one, attn=None, contrib=None, top_slot=one, top_value=one, G=2, P=5, H=8,
                A=8, D=8, scale=1.0, alpha_s=0.0, beta_s=0.0, use_weight=0, use_penalty=0, stream=None)
    call = lambda **kw: getattr(lib, NAME)(*dict(base, **kw).values())
    err = lib.lime_last_error_string
    assert call(by=2) == -1 and b'LIME_EXPLAIN_BY' in err()
    for name in ('kp', 'g', 'qp', 'cand', 'offsets', 'logits', 'base', 'weight', 'top_slot', 'top_value'):
        assert call(**{name: None}) == -1 and b'NULL' in err(), name
    assert call(occ=one) == -1 and call(index=one, n=3, occ=one, qt=one) == -1 and call(occ=one, qt=one, ct=one, n_occ=2) == -1
    assert b'together' in err()
    assert call(use_weight=1) == -1 and b'remaining' in err()
    assert call(H=129) == -2 and call(H=0) == -1 and call(A=6) == -2 and call(D=2052) == -2
    assert call(kp=ctypes.c_void_p(20)) == -1 and b'16-byte aligned' in err()
    assert call(index=one, n=0) == -1 and b'empty table' in err()
    assert call(index=one, n=3, occ=one, qt=one, ct=one, n_occ=0) == -1 and b'empty occurrence table' in err()
    assert call(m=0) == -1 and call(m=9) == -1 and call(hist_div=0) == -1            # m > H = 8
    assert call(m=17, H=32) == -2 and b'16' in err()
    assert call(m=17, H=16) == -1                                                    # m > H is refused first
    assert call(G=0) == 0 and call(P=0) == 0                                         # nothing to do: no launch


# ---- the host refusals of the model's entries ------------------------------------------------------------------------------------------
def fake_corpus(n_news=20, topics=3):
    ids = torch.arange(n_news, dtype=torch.int32)
    return types.SimpleNamespace(news_category=ids % topics, news_subCategory=torch.zeros(n_news, dtype=torch.int32))


def list_args(U=3, Hh=6, lens=(2, 0, 3), n_news=20):
    P = sum(lens)
    return dict(news_cache=torch.zeros(n_news, 8), corpus=fake_corpus(n_news), hist_index=torch.zeros(U, Hh, dtype=torch.int32),
                hist_mask=torch.ones(U, Hh, dtype=torch.bool), user_freshness=torch.zeros(U, Hh), user_lifetime=torch.zeros(U, Hh),
                cand_offsets=torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64),
                cand_index=torch.arange(P, dtype=torch.int32), cand_freshness=torch.zeros(P), cand_lifetime=torch.zeros(P))


def pool_args(U=3, Hh=6, C=5, k=2, n_news=20):
    a = list_args(U, Hh, (0,) * U, n_news)
    del a['cand_offsets']
    return dict(a, cand_index=torch.arange(C, dtype=torch.int32), cand_freshness=torch.zeros(C), cand_lifetime=torch.zeros(U, C),
                positions=torch.zeros(U, k, dtype=torch.int32))


def both(model, **kw):
    """The two entries on arguments that are fine up to ``kw``."""
    return (lambda: model.explain_lists(**list_args(), **kw)), (lambda: model.explain(**pool_args(), **kw))


@pytest.fixture(autouse=True)
def no_launch(monkeypatch):
    """A refusal comes before any launch: with the library out of reach, a launch would raise something else."""
    def refuse():
        raise AssertionError('the library was reached before the refusal')
    monkeypatch.setattr(_lib, 'load', refuse)
    yield


@pytest.mark.parametrize('top', [0, -1, 7, 17, 2.0, True, None])
def test_top_outside_its_range_is_refused(top, monkeypatch):
    model = Model(make_config(**_TINY))
    for call in both(model, top=top):
        with pytest.raises(ValueError, match=r'top must be an integer in 1 \.\. min\(16, H\)'):
            call()


def test_an_unknown_by_is_refused():
    model = Model(make_config(**_TINY))
    for call in both(model, by='gradient'):
        with pytest.raises(ValueError, match="by must be 'contribution' or 'attention'"):
            call()


def test_contribution_under_the_mlp_predictor_is_refused():
    model = Model(make_config(click_predictor='mlp', **_TINY))
    for call in both(model) + both(model, by='contribution'):
        with pytest.raises(ValueError, match='ReLU'):
            call()


def test_cne_is_refused_with_score_pools_message():
    model = Model(make_config(content_encoder='CNE', **_TINY))
    for call in both(model) + both(model, top=99):
        with pytest.raises(ValueError, match='CNE') as e:
            call()
        assert str(e.value) == model._NO_CONTENT_CACHE


@pytest.mark.parametrize('change,match', [
    (dict(hist_index=torch.zeros(3, dtype=torch.int32)), r'hist_index must be \[U, H\]'),
    (dict(hist_mask=torch.ones(3, 5, dtype=torch.bool)), 'hist_mask must be'),
    (dict(cand_offsets=torch.tensor([0, 2, 2, 4])), 'end at P = 5'),
    (dict(cand_freshness=torch.zeros(4)), 'cand_freshness must be'),
    (dict(pairs_per_pass=0), 'pairs_per_pass must be positive'),
])
def test_explain_lists_has_score_lists_refusals(change, match):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match=match):
        model.explain_lists(**dict(list_args(), **change))


@pytest.mark.parametrize('change,match', [
    (dict(hist_index=torch.zeros(3, dtype=torch.int32)), r'hist_index must be \[U, H\]'),
    (dict(cand_index=torch.zeros(1, 5, dtype=torch.int32)), r'cand_index must be \[C\]'),
    (dict(positions=torch.zeros(2, 2, dtype=torch.int32)), r'positions must be the int \[U, k\]'),
    (dict(positions=torch.zeros(3, 2)), r'positions must be the int \[U, k\]'),
    (dict(positions=[[0, 1]] * 3), r'positions must be the int \[U, k\]'),
    (dict(cand_freshness=torch.zeros(4)), 'cand_freshness must be'),
    (dict(cand_lifetime=torch.zeros(2, 5)), 'cand_lifetime must be'),
    (dict(hist_mask=torch.ones(3, 5, dtype=torch.bool)), 'hist_mask must be'),
])
def test_explain_refuses_bad_pool_arguments(change, match):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match=match):
        model.explain(**dict(pool_args(), **change))


def test_no_pairs_give_an_empty_record():
    model = Model(make_config(**_TINY))
    ex = model.explain_lists(**list_args(lens=(0, 0, 0)), top=2, dense=True)
    assert ex.score.shape == (0,) and ex.slots.shape == (0, 2) and ex.slots.dtype == torch.int32 and ex.attention.shape == (0, 6)
