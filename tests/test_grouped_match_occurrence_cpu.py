"""The occurrence-composed grouped matches without a GPU: what lime_grouped_match_occurrence_f32 and
lime_grouped_mlp_match_occurrence_f32 refuse before any launch (the statuses and their order, following
tests/test_abi.py::test_bad_arguments_are_rejected_without_a_launch -- no pointer is read, so plain addresses stand for the buffers), and
Model.occurrence_match_applicable() over the configurations."""
import pytest

from lime_cikm25_amd import Model, _lib, make_config, model as model_module, ops
from lime_cikm25_amd.build import build_library
from user_cases import _TINY

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2
AT = 0x10000                               # a 16-byte aligned address: the entries check pointers, they do not read them here


@pytest.fixture(scope='module')
def lib():
    build_library()
    return _lib.load()


def dot(lib, H=4, A=8, D=8, n=1, n_occ=1, P=1, G=1, use_weight=0, **ptr):
    p = dict(kp=AT, g=AT, qa=AT, ca=AT, qt=AT, ct=AT, remaining=None, offsets=AT, index=AT, occ=AT, logits=AT)
    p.update(ptr)
    return lib.lime_grouped_match_occurrence_f32(p['kp'], p['g'], p['qa'], p['ca'], p['qt'], p['ct'], p['remaining'], p['offsets'], p['index'], n,
                                                 p['occ'], n_occ, p['logits'], G, P, H, A, D, 1.0, 0.0, 0.0, use_weight, 0, None)


def mlp(lib, H=4, A=8, D=8, n=1, n_occ=1, P=1, G=1, **ptr):
    p = dict(kp=AT, gu=AT, qa=AT, na=AT, qt=AT, nt=AT, w_out=AT, b_out=AT, offsets=AT, index=AT, occ=AT, logits=AT)
    p.update(ptr)
    return lib.lime_grouped_mlp_match_occurrence_f32(p['kp'], p['gu'], p['qa'], p['na'], p['qt'], p['nt'], p['w_out'], p['b_out'], p['offsets'],
                                                     p['index'], n, p['occ'], n_occ, p['logits'], G, P, H, A, D, 1.0, None)


@pytest.mark.parametrize('entry,second,second_occ', [(dot, 'ca', 'ct'), (mlp, 'na', 'nt')])
def test_refusals_come_back_with_their_status_and_no_launch(lib, entry, second, second_occ):
    # NULL index, occ or table
    for name in ('index', 'occ', 'qa', second, 'qt', second_occ):
        assert entry(lib, **{name: None}) == BAD_ARG, name
        assert b'NULL' in lib.lime_last_error_string()
    # an empty news table or an empty occurrence table under pairs; no pairs: nothing to read, and nothing launched
    assert entry(lib, n=0) == BAD_ARG and b'empty table' in lib.lime_last_error_string()
    assert entry(lib, n_occ=0) == BAD_ARG and b'empty occurrence table' in lib.lime_last_error_string()
    assert entry(lib, n=0, n_occ=0, P=0) == OK
    assert entry(lib, n=-1) == BAD_ARG and entry(lib, n_occ=-1) == BAD_ARG
    # a table off its grid: 16 bytes, 8 bytes for na / nt
    for name in ('qa', 'qt'):
        assert entry(lib, **{name: AT + 8}) == BAD_ARG, name
        assert b'aligned' in lib.lime_last_error_string()
    for name in (second, second_occ):
        assert entry(lib, **{name: AT + (8 if entry is dot else 4)}) == BAD_ARG, name
        assert b'aligned' in lib.lime_last_error_string()
    # dims outside the plain kernels' limits
    for H, A, D in ((129, 8, 8), (4, 2052, 8), (4, 8, 2052), (4, 6, 8), (4, 8, 7)):
        assert entry(lib, H=H, A=A, D=D) == UNSUPPORTED, (H, A, D)
    assert entry(lib, n=1 << 31) == UNSUPPORTED and entry(lib, n_occ=1 << 31) == UNSUPPORTED
    # the order of the indexed entries: NULL before the dims, the dims before the alignment, the alignment before the empty tables
    assert entry(lib, H=129, index=None) == BAD_ARG
    assert entry(lib, H=129, qt=AT + 4) == UNSUPPORTED
    assert entry(lib, n_occ=0, qt=AT + 4) == BAD_ARG and b'aligned' in lib.lime_last_error_string()
    assert entry(lib, n=0, n_occ=0) == BAD_ARG and b'empty table' in lib.lime_last_error_string()


def test_the_dot_product_entry_needs_remaining_under_the_weight(lib):
    assert dot(lib, use_weight=1) == BAD_ARG and b'remaining' in lib.lime_last_error_string()
    assert dot(lib, use_weight=1, index=None) == BAD_ARG and b'NULL pointer' in lib.lime_last_error_string()


def test_the_abi_version_is_that_of_the_indexed_entries(lib):
    """The two entries are additions: no existing signature moved, the version stays."""
    assert lib.lime_abi_version() == _lib.ABI_VERSION == 14


APPLICABLE = {
    # fusion method x projection / identity
    'concat_project': (dict(), True),
    'concat_identity': (dict(lime_output_dim=0), False),                   # columns are concatenated, not added
    'add': (dict(fusion_method='add'), True),
    'add_without_projection': (dict(fusion_method='add', lime_output_dim=0), True),      # 'add' never projects: the dim is not read
    'gated': (dict(fusion_method='gated'), False),                         # not linear in the occurrence
    # the three user encoders and both click predictors
    'att_user': (dict(user_encoder='ATT'), True),
    'mhsa_user': (dict(user_encoder='MHSA'), True),
    'mlp_crown_user': (dict(click_predictor='mlp'), True),
    'mlp_att_user': (dict(user_encoder='ATT', click_predictor='mlp'), True),
    'mlp_mhsa_add': (dict(user_encoder='MHSA', click_predictor='mlp', fusion_method='add'), True),
    'mlp_gated': (dict(click_predictor='mlp', fusion_method='gated'), False),
    'attention_off': (dict(use_candidate_ware_clicked_news_attention=False), True),
    'other_content_encoder': (dict(content_encoder='NAML', user_encoder='ATT'), True),
    # CNE has no cache; a baseline model has no occurrence (it keeps its indexed path)
    'cne': (dict(content_encoder='CNE'), False),
    'baseline_crown': (dict(news_encoder='CROWN'), False),
    'baseline_naml_att': (dict(news_encoder='NAML', user_encoder='ATT'), False),
}


@pytest.mark.parametrize('name', list(APPLICABLE))
def test_occurrence_match_applicable(name, monkeypatch):
    kw, want = APPLICABLE[name]
    model = Model(make_config(**{**_TINY, **kw}))
    assert model.occurrence_match_applicable() is want
    # a predicate of the configuration: the switch is not part of it, the composed MLP form (the yardstick on existing launches) is
    monkeypatch.setattr(model_module, 'OCCURRENCE_MATCH', not model_module.OCCURRENCE_MATCH)
    assert model.occurrence_match_applicable() is want
    monkeypatch.setattr(ops, 'FUSED_MLP_MATCH', False)
    assert model.occurrence_match_applicable() is (want and model.click_predictor != 'mlp')


def test_the_switch_is_off_by_default():
    import os
    assert model_module.OCCURRENCE_MATCH is (os.environ.get('LIME_OCCURRENCE_MATCH', '0') != '0')
