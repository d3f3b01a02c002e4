"""Schedules without a GPU: the host-side refusals of Model.score_schedule / Model.recommend_schedule (score_pool's, in its order, and
the two of ``slot_offsets``), what lime_grouped_match_schedule_f32 refuses before any launch (statuses and their order, in the manner
of tests/test_grouped_match_occurrence_cpu.py: no pointer is read, so plain addresses stand for the buffers) and the route predicate
over the configurations."""
import subprocess

import pytest
import torch

from lime_cikm25_amd import Model, _lib, make_config, model as model_module, ops
from lime_cikm25_amd.build import build_library
from test_recommend_cpu import pool_args
from user_cases import _TINY

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
AT = 0x10000                               # a 16-byte aligned address: the entry checks pointers, it does not read them here


def schedule_args(S=3, **kw):
    return dict(pool_args(**kw), slot_offsets=torch.arange(S, dtype=torch.float32))


# ---- host-side refusals --------------------------------------------------------------------------------------------------------------
def test_cne_is_refused_with_the_pool_s_words():
    model = Model(make_config(content_encoder='CNE', **_TINY))
    assert 'no per-news content cache' in Model._NO_CONTENT_CACHE
    for call in (lambda: model.score_schedule(**schedule_args()), lambda: model.recommend_schedule(k=2, **schedule_args())):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == Model._NO_CONTENT_CACHE


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
    # the schedule's own
    (dict(slot_offsets=torch.zeros(2, 3)), r'slot_offsets must be a float \[S\] with S >= 1'),
    (dict(slot_offsets=torch.tensor(1.0)), r'slot_offsets must be a float \[S\] with S >= 1'),
    (dict(slot_offsets=torch.zeros(0)), r'slot_offsets must be a float \[S\] with S >= 1'),
    (dict(slot_offsets=torch.zeros(3, dtype=torch.int64)), r'slot_offsets must be a float \[S\]'),
])
def test_bad_arguments_are_value_errors_on_the_host(change, match):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match=match):
        model.score_schedule(**dict(schedule_args(), **change))
    with pytest.raises(ValueError, match=match):
        model.recommend_schedule(k=1, **dict(schedule_args(), **change))


def test_the_pool_s_refusals_come_before_the_schedule_s():
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match='cand_freshness must be'):
        model.score_schedule(**dict(schedule_args(), cand_freshness=torch.zeros(4), slot_offsets=torch.zeros(0)))
    with pytest.raises(ValueError, match='slot_offsets must be'):
        model.recommend_schedule(k=0, **dict(schedule_args(), slot_offsets=torch.zeros(0)))


@pytest.mark.parametrize('k', [0, -1, 129])
def test_k_out_of_range_is_a_value_error(k):
    model = Model(make_config(**_TINY))
    with pytest.raises(ValueError, match='recommend_schedule keeps 1 <= k <= 128'):
        model.recommend_schedule(k=k, **schedule_args())


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def entry(lib, H=4, A=8, D=8, n=1, n_occ=1, P=1, G=1, S=2, use_weight=0, **ptr):
    p = dict(kp=AT, g=AT, qa=AT, ca=AT, qt=AT, ct=AT, remaining=None, offsets=AT, index=AT, occ=AT, logits=AT)
    p.update(ptr)
    return lib.lime_grouped_match_schedule_f32(p['kp'], p['g'], p['qa'], p['ca'], p['qt'], p['ct'], p['remaining'], p['offsets'], p['index'], n,
                                               p['occ'], n_occ, p['logits'], G, P, S, H, A, D, 1.0, 0.0, 0.0, use_weight, 0, None)


BASELINE = dict(qt=None, ct=None, occ=None, n_occ=0)


def test_the_symbol_is_declared_bound_and_exported(lib):
    name = 'lime_grouped_match_schedule_f32'
    exported = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert name + '(' in open(_lib.HEADER_PATH).read()
    assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert (' T ' + name + '\n') in exported
    assert lib.lime_abi_version() == _lib.ABI_VERSION == 14         # an addition: no existing signature moved


def test_the_twin_s_refusals_in_the_twin_s_order(lib):
    for name in ('index', 'kp', 'g', 'qa', 'ca', 'offsets', 'logits'):
        assert entry(lib, **{name: None}) == BAD_ARG, name
        assert b'NULL pointer' in lib.lime_last_error_string()
    assert entry(lib, use_weight=1) == BAD_ARG and b'remaining' in lib.lime_last_error_string()
    assert entry(lib, use_weight=1, index=None) == BAD_ARG and b'NULL pointer' in lib.lime_last_error_string()
    assert entry(lib, n=0) == BAD_ARG and b'empty table' in lib.lime_last_error_string()
    assert entry(lib, n_occ=0) == BAD_ARG and b'empty occurrence table' in lib.lime_last_error_string()
    assert entry(lib, n=0, n_occ=0, P=0) == OK
    assert entry(lib, n=-1) == BAD_ARG and entry(lib, n_occ=-1) == BAD_ARG
    for H, A, D in ((0, 8, 8), (4, 0, 8), (4, 8, -4)):
        assert entry(lib, H=H, A=A, D=D) == BAD_ARG and b'bad dims' in lib.lime_last_error_string()
    for name in ('kp', 'g', 'qa', 'ca', 'qt', 'ct'):
        assert entry(lib, **{name: AT + 8}) == BAD_ARG, name
        assert b'aligned' in lib.lime_last_error_string()
    for H, A, D in ((129, 8, 8), (4, 2052, 8), (4, 8, 2052), (4, 6, 8), (4, 8, 7)):
        assert entry(lib, H=H, A=A, D=D) == UNSUPPORTED, (H, A, D)
        assert b'multiples of 4' in lib.lime_last_error_string()
    assert entry(lib, n=1 << 31) == UNSUPPORTED and entry(lib, n_occ=1 << 31) == UNSUPPORTED
    # NULL before the dims, the dims before the alignment, the alignment before the empty tables
    assert entry(lib, H=129, index=None) == BAD_ARG
    assert entry(lib, H=129, qt=AT + 4) == UNSUPPORTED
    assert entry(lib, n_occ=0, qt=AT + 4) == BAD_ARG and b'aligned' in lib.lime_last_error_string()
    assert entry(lib, n=0, n_occ=0) == BAD_ARG and b'empty table' in lib.lime_last_error_string()


def test_the_schedule_s_own_refusals_come_behind_them(lib):
    for S in (0, -3):
        assert entry(lib, S=S) == BAD_ARG and b'slots' in lib.lime_last_error_string()
    assert entry(lib, occ=None) == BAD_ARG and b'without occ' in lib.lime_last_error_string()
    assert entry(lib, qt=None) == BAD_ARG and b'come together' in lib.lime_last_error_string()
    assert entry(lib, ct=None) == BAD_ARG and b'come together' in lib.lime_last_error_string()
    assert entry(lib, qt=None, ct=None, occ=None, n_occ=3) == BAD_ARG and b'need them' in lib.lime_last_error_string()
    # behind the twin's: an empty news table, a bad dim and an unsupported H are named first
    assert entry(lib, S=0, n=0) == BAD_ARG and b'empty table' in lib.lime_last_error_string()
    assert entry(lib, S=0, H=129) == UNSUPPORTED
    assert entry(lib, S=0, occ=None) == BAD_ARG and b'slots' in lib.lime_last_error_string()          # S before occ
    # the baseline form: no tables, no occ, n_occ = 0 -- accepted (no pairs: nothing launched)
    assert entry(lib, P=0, **BASELINE) == OK and entry(lib, G=0, **BASELINE) == OK
    assert entry(lib, S=0, P=0, **BASELINE) == BAD_ARG


@pytest.mark.parametrize('H,n_occ,fits', [
    (50, 100, True),                 # the defaults: 8192 + 8 * 100 * 52 = 49,792 bytes
    (64, 100, True), (64, 112, True), (64, 113, False),
    (1, 100, True), (1, 1984, True), (1, 1985, False),
    (16, 496, True), (16, 497, False), (32, 240, True), (32, 241, False),
    (128, 48, True), (128, 49, False), (65, 100, False), (128, 100, False),
    (128, 0, True), (50, 0, True),
])
def test_the_lds_bound_is_the_one_the_host_predicate_states(lib, H, n_occ, fits):
    """2048 T + 8 n_occ Hs <= 65536: the entry's status (no pairs, so nothing is launched when it fits) and
    ops.grouped_match_schedule_fits agree at both sides of every threshold."""
    kw = dict(BASELINE) if n_occ == 0 else dict(n_occ=n_occ)
    assert entry(lib, H=H, P=0, **kw) == (OK if fits else UNSUPPORTED)
    if not fits:
        assert b'bytes of LDS' in lib.lime_last_error_string()
    assert ops.grouped_match_schedule_fits(H, n_occ) is fits
    assert ops.grouped_match_schedule_fits(129, 0) is False and ops.grouped_match_schedule_fits(0, 0) is False


# ---- the route -----------------------------------------------------------------------------------------------------------------------
ROUTES = {
    # name: (configuration, schedule_match_applicable(), route of a 3-slot schedule)
    'concat_project': (dict(), True, 'factorised'),
    'add': (dict(fusion_method='add'), True, 'factorised'),
    'att_user': (dict(user_encoder='ATT'), True, 'factorised'),
    'mhsa_user': (dict(user_encoder='MHSA'), True, 'factorised'),
    'attention_off': (dict(use_candidate_ware_clicked_news_attention=False), True, 'factorised'),
    'other_content_encoder': (dict(content_encoder='NAML', user_encoder='ATT'), True, 'factorised'),
    'fixed_lifetime': (dict(lifetime_type='fixed'), True, 'factorised'),
    # a baseline: no occurrence tables, only the weight moves
    'baseline_crown': (dict(news_encoder='CROWN'), True, 'factorised'),
    'baseline_naml_att': (dict(news_encoder='NAML', user_encoder='ATT'), True, 'factorised'),
    # not linear in the occurrence / concatenated columns: the shared user side
    'gated': (dict(fusion_method='gated'), False, 'shared'),
    'concat_identity': (dict(lime_output_dim=0), False, 'shared'),
    # the MLP predictor: its pooled hidden row depends on the slot through the softmax
    'mlp_crown_user': (dict(click_predictor='mlp'), False, 'shared'),
    'mlp_att_add': (dict(user_encoder='ATT', click_predictor='mlp', fusion_method='add'), False, 'shared'),
    'mlp_gated': (dict(click_predictor='mlp', fusion_method='gated'), False, 'shared'),
    # ... and a baseline under it reads no time at all
    'mlp_baseline': (dict(news_encoder='NAML', user_encoder='ATT', click_predictor='mlp'), False, 'expand'),
    'mlp_baseline_crown': (dict(news_encoder='CROWN', click_predictor='mlp'), False, 'expand'),
    # beyond the kernel's LDS bound: 100 occurrences x 128 history rows (the ATT user encoder matches ONE pooled row: inside)
    'long_history': (dict(max_history_num=128), False, 'shared'),
    'long_history_att': (dict(max_history_num=128, user_encoder='ATT'), True, 'factorised'),
    'long_history_baseline': (dict(max_history_num=128, news_encoder='CROWN'), True, 'factorised'),
    'many_buckets': (dict(num_buckets=13), False, 'shared'),                  # 169 x 52 rows at H = 50
    'defaults': (dict(max_history_num=50, num_buckets=10), True, 'factorised'),
}


@pytest.mark.parametrize('name', list(ROUTES))
def test_the_route_is_a_pure_function_of_the_configuration(name, monkeypatch):
    kw, applicable, route = ROUTES[name]
    cfg = {**_TINY, **kw}
    if name == 'many_buckets':
        cfg['max_history_num'] = 50
    model = Model(make_config(**cfg))
    assert model.schedule_match_applicable() is applicable
    assert model.schedule_route(3) == route and model.schedule_route(24) == route
    assert model.schedule_route(1) == 'single'
    # the other switches are not read; LIME_SCHEDULE_MATCH=0 sends the factorised models to the shared user side, and only them
    for switch in ('OCCURRENCE_MATCH', 'INDEXED_MATCH'):
        monkeypatch.setattr(model_module, switch, not getattr(model_module, switch))
        assert model.schedule_match_applicable() is applicable and model.schedule_route(3) == route
    monkeypatch.setattr(model_module, 'SCHEDULE_MATCH', False)
    assert model.schedule_match_applicable() is applicable
    assert model.schedule_route(3) == ('shared' if route == 'factorised' else route) and model.schedule_route(1) == 'single'


def test_the_history_length_of_the_call_decides_not_the_configured_one():
    model = Model(make_config(**_TINY))
    assert model.schedule_route(3, H=64) == 'factorised' and model.schedule_route(3, H=65) == 'shared'
    assert Model(make_config(**{**_TINY, 'user_encoder': 'ATT'})).schedule_route(3, H=128) == 'factorised'


def test_the_switch_is_on_by_default():
    import os
    assert model_module.SCHEDULE_MATCH is (os.environ.get('LIME_SCHEDULE_MATCH', '1') != '0')
