"""The MLP click predictor (config.click_predictor = 'mlp'; reference model.py:113-115, :139-141, :182-184) on the CPU: every supported
pairing builds with it, the state_dict and the trainable set are the reference's key for key (tests/golden/mlp_*.npz,
tools/make_mlp_goldens.py), a reference-layout checkpoint loads strictly, the reference's other click predictors stay refused with
their reason, and the parameters the training step leaves out are exactly the ones the reference's backward leaves without a
gradient.  No GPU."""
import json

import pytest
import torch

import mlp_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, make_config, training

CONTENT = ['CROWN', 'CNN', 'NAML', 'MHSA', 'CNE', 'KCNN']
USERS = ['CROWN', 'ATT', 'MHSA']
PLAIN = [(n, u) for n in ('CROWN', 'CNN', 'NAML', 'MHSA', 'KCNN') for u in ('ATT', 'MHSA')] + [('CROWN', 'CROWN')]
NEW_KEYS = ['mlp.weight', 'mlp.bias', 'out.weight', 'out.bias']


def _check_predictor(model):
    D = model.news_embedding_dim
    assert model.click_predictor == 'mlp'
    assert tuple(model.mlp.weight.shape) == (D // 2, 2 * D) and tuple(model.mlp.bias.shape) == (D // 2,)
    assert tuple(model.out.weight.shape) == (1, D // 2) and tuple(model.out.bias.shape) == (1,)
    assert list(model.state_dict())[-4:] == NEW_KEYS                       # where the reference constructs them: last
    out_before = model.out.weight.detach().clone()
    model.initialize()
    assert float(model.mlp.bias.detach().abs().max()) == 0.0               # model.py:139-141
    bound = (2.0 ** 0.5) * (6.0 / (D // 2 + 2 * D)) ** 0.5                 # xavier_uniform_ with the ReLU gain
    assert 0.5 * bound < float(model.mlp.weight.detach().abs().max()) <= bound * (1 + 1e-6)
    assert torch.equal(model.out.weight, out_before)                       # ``out`` keeps nn.Linear's default initialisation


@pytest.mark.parametrize('user', USERS)
@pytest.mark.parametrize('content', CONTENT)
def test_every_lime_pairing_builds_with_the_mlp_predictor(content, user):
    model = Model(make_config(content_encoder=content, user_encoder=user, click_predictor='mlp', vocabulary_size=500))
    assert model.model_name == 'LIME-%s-%s' % (content, user)
    _check_predictor(model)


@pytest.mark.parametrize('news,user', PLAIN)
def test_every_baseline_pairing_builds_with_the_mlp_predictor(news, user):
    model = Model(make_config(news_encoder=news, user_encoder=user, click_predictor='mlp', vocabulary_size=500))
    assert model.model_name == '%s-%s' % (news, user)
    _check_predictor(model)


def test_the_dot_product_model_has_no_predictor_parameters():
    model = Model(make_config(vocabulary_size=500))
    assert model.click_predictor == 'dot_product' and not hasattr(model, 'mlp') and not hasattr(model, 'out')
    assert not [k for k in model.state_dict() if k.startswith(('mlp.', 'out.'))]


@pytest.mark.parametrize('name', list(mlp_cases.CASES))
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = mlp_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    spec = json.loads(str(g['state_dict_spec']))
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == spec
    assert [k for k, _ in spec][-4:] == NEW_KEYS
    if model.model_name == 'LIME-CROWN-CROWN':
        assert len(spec) == 187 and [k for k, _ in spec].index('mlp.weight') == 183
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))
    assert set(NEW_KEYS) <= set(json.loads(str(g['trainable'])))


@pytest.mark.parametrize('name', list(mlp_cases.CASES))
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = mlp_cases.build_case(name)
    sd = synth_state_dict(json.loads(str(load_golden(name)['state_dict_spec'])))
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    for k in NEW_KEYS:
        assert torch.equal(model.state_dict()[k], sd[k])
    # the checkpoint of the dot-product model lacks the four tensors: a strict load says so
    plain = {k: v for k, v in sd.items() if k not in NEW_KEYS}
    with pytest.raises(RuntimeError, match='mlp.weight'):
        Model(cfg).load_state_dict(plain, strict=True)


@pytest.mark.parametrize('predictor,why', [('sigmoid', 'no branch'), ('FIM', 'HDC')])
def test_the_other_click_predictors_stay_refused(predictor, why):
    with pytest.raises(NotImplementedError, match='dot_product .* and mlp') as e:
        Model(make_config(click_predictor=predictor, vocabulary_size=500))
    assert repr(predictor) in str(e.value) and why in str(e.value)


@pytest.mark.parametrize('name', mlp_cases.GRAD_CASES)
def test_dead_parameters_are_the_ones_the_reference_gives_no_gradient(name):
    cfg, _, _ = mlp_cases.build_case(name)
    g = load_golden('grad_' + name)
    model = Model(cfg)
    without = json.loads(str(g['without_grad']))
    # without_grad lists every parameter whose .grad stayed None: the frozen tables (requires_grad False) and the dead ones
    frozen = [k for k, p in dict(model.named_parameters()).items() if not p.requires_grad and k in without]
    dead = training.dead_parameters(model)
    assert sorted(dead + frozen) == sorted(without)
    assert not set(dead) & set(frozen)
    names = training.TrainStep.bucket_names(model)
    assert names == json.loads(str(g['with_grad']))                        # the bucket: the reference's gradients, in its order
    assert names[-4:] == NEW_KEYS                                          # all four new tensors receive gradients
    # the same rule as for the dot-product model: the predictor changes no other parameter's fate
    same = Model(make_config(**dict(mlp_cases.CASES[name]['cfg'], click_predictor='dot_product')))
    assert training.dead_parameters(same) == dead


@pytest.mark.parametrize('name', mlp_cases.GRAD_CASES)
def test_a_gradient_golden_pins_the_predictor(name):
    g = load_golden('grad_' + name)
    for k in NEW_KEYS[:3]:
        assert float(g['norm:' + k]) > 0.0, k
    # out.bias: identically zero (a constant added to every logit of a row leaves the softmax loss alone); the golden holds the
    # reference's rounding residue, far under one fp32 epsilon per logit
    assert float(abs(g['full:out.bias']).max()) <= g['logits'].size * 2.0 ** -23
