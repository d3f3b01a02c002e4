"""The category-prediction loss of the bare CROWN baselines (``config.alpha``), the parts that need no GPU: which parameters train, the
attribute after construction, the kernel's declaration and the wrapper's host checks.  The goldens (tests/golden/grad_aux_*.npz) are the
reference's, tools/make_aux_goldens.py."""
import json
import re

import pytest
import torch

import aux_cases
import plain_cases
from helpers import load_golden
from test_abi import HEADER, declared_symbols
from lime_cikm25_amd import Model, _lib, ops, training


def _lists(model, g):
    without = json.loads(str(g['without_grad']))
    frozen = [k for k, p in dict(model.named_parameters()).items() if not p.requires_grad and k in without]
    return json.loads(str(g['with_grad'])), without, frozen


@pytest.mark.parametrize('name', list(aux_cases.CASES))
def test_dead_parameters_and_the_bucket_are_the_references(name):
    cfg, _, _ = aux_cases.build_case(name)
    model = Model(cfg)
    with_grad, without, frozen = _lists(model, load_golden('grad_' + name))
    dead = training.dead_parameters(model)
    assert sorted(dead + frozen) == sorted(without) and not set(dead) & set(frozen)
    assert training.TrainStep.bucket_names(model) == with_grad
    bare = name in aux_cases.BARE_CASES
    assert training.trains_category_predictor(model) == bare
    assert all((k in with_grad) == bare for k in aux_cases.FC)
    fc = [k for k in dead if 'category_predictor.' in k]
    assert fc == ([] if bare else ['news_encoder.base_news_encoder.category_predictor.fc.weight',
                                   'news_encoder.base_news_encoder.category_predictor.fc.bias'])


@pytest.mark.parametrize('alpha', [0, 0.0])
def test_alpha_zero_changes_nothing(alpha):
    """plain_crown_crown's golden was made with the default alpha = 0: the same dead list and the same bucket."""
    cfg, _, _ = plain_cases.build_case('plain_crown_crown')
    assert cfg.alpha == 0
    cfg.alpha = alpha
    model = Model(cfg)
    with_grad, without, frozen = _lists(model, load_golden('grad_plain_crown_crown'))
    assert not training.trains_category_predictor(model)
    assert sorted(training.dead_parameters(model) + frozen) == sorted(without)
    assert training.TrainStep.bucket_names(model) == with_grad and not set(aux_cases.FC) & set(with_grad)


@pytest.mark.parametrize('name', list(aux_cases.CASES))
def test_the_attribute_is_none_after_construction(name):
    cfg, _, _ = aux_cases.build_case(name)
    model = Model(cfg)
    assert model.news_encoder.auxiliary_loss is None
    assert getattr(model.news_encoder, 'base_news_encoder', model.news_encoder).auxiliary_loss is None
    assert model.content_encoder.alpha == cfg.alpha


def test_the_goldens_hold_a_term_that_is_not_the_candidates():
    for name in aux_cases.CASES:
        g = load_golden('grad_' + name)
        assert bool(g['aux_none']) == (name not in aux_cases.BARE_CASES)
        assert abs(float(g['nll']) + float(g['aux']) - float(g['loss'])) < 1e-5 * float(g['loss'])
        if name in aux_cases.BARE_CASES:
            assert float(g['aux']) > 0.1 and abs(float(g['aux']) - float(g['aux_candidates'])) > 0.05 * float(g['aux'])
            assert all(float(g['norm:' + k]) > 0 for k in aux_cases.FC)


def test_the_header_declares_the_entry():
    assert 'lime_linear_xent_f32' in declared_symbols() and 'lime_linear_xent_f32' in _lib.SIGNATURES
    res, args = _lib.SIGNATURES['lime_linear_xent_f32']
    assert len(args) == 14
    text = open(HEADER).read()
    assert re.search(r'#define\s+LIME_ABI_VERSION\s+14\b', text), 'an added entry leaves the ABI version alone'


def test_the_wrapper_checks_on_the_host():
    x, w, t = torch.zeros(4, 8), torch.zeros(3, 8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match='2-D'):
        ops.linear_xent(x[0], w, None, t, 1.0)
    with pytest.raises(ValueError, match='columns'):
        ops.linear_xent(x, torch.zeros(3, 9), None, t, 1.0)
    with pytest.raises(ValueError, match='C <= 1024'):
        ops.linear_xent(x, torch.zeros(1025, 8), None, t, 1.0)
    with pytest.raises(ValueError, match='C <= 1024'):
        ops.linear_xent(x, torch.zeros(0, 8), None, t, 1.0)
    with pytest.raises(ValueError, match='M >= 1'):
        ops.linear_xent(x[:0], w, None, t[:0], 1.0)
    with pytest.raises(TypeError, match='int32'):
        ops.linear_xent(x, w, None, t.long(), 1.0)
    with pytest.raises(TypeError, match='int32'):
        ops.linear_xent(x, w, None, None, 1.0)
    with pytest.raises(ValueError, match='elements'):
        ops.linear_xent(x, w, None, t[:3], 1.0)
    with pytest.raises(ValueError, match='elements'):
        ops.linear_xent(x, w, torch.zeros(4), t, 1.0)
    with pytest.raises(TypeError, match='CUDA'):                     # well-formed, but on the host: there is no CPU fallback
        ops.linear_xent(x, w, torch.zeros(3), t, 1.0)
