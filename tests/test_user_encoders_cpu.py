"""The ATT and MHSA user encoders (config.user_encoder) on the CPU: every pairing with the four content encoders builds, the other user
encoders of the reference stay refused, the state_dict is the reference's key for key and shape for shape (tests/golden/user_*.npz,
tools/make_user_goldens.py), a reference-layout checkpoint loads strictly, and the parameters the training step leaves out are exactly
the ones the reference's backward leaves without a gradient.  No GPU."""
import json

import pytest
import torch

import golden_cases
import user_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, make_config, training


@pytest.mark.parametrize('content', ['CROWN', 'CNN', 'NAML', 'MHSA'])
@pytest.mark.parametrize('user', ['CROWN', 'ATT', 'MHSA'])
def test_every_pairing_builds(content, user):
    model = Model(make_config(content_encoder=content, user_encoder=user, vocabulary_size=500))
    assert model.model_name == 'LIME-%s-%s' % (content, user)
    assert type(model.user_encoder).__name__ == user
    keys = [k for k in model.state_dict() if k.startswith('user_encoder.') and not k.startswith('user_encoder.news_encoder.')]
    has = lambda s: any(k.startswith('user_encoder.' + s) for k in keys)
    assert has('graph_sage') == has('user_node_embedding') == has('K.') == has('Q.') == (user == 'CROWN')
    assert has('multiheadAttention.') == (user == 'MHSA')
    assert has('attention.affine2.') == (user != 'CROWN')


@pytest.mark.parametrize('user', ['LSTUR', 'GRU', 'PUE', 'CATT', 'MINER', 'SUE', 'FIM'])
def test_other_user_encoders_stay_refused(user):
    with pytest.raises(NotImplementedError, match='ATT, CROWN, MHSA'):
        Model(make_config(user_encoder=user, vocabulary_size=500))


@pytest.mark.parametrize('name', list(user_cases.CASES))
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = user_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))


def test_user_side_keys_in_the_reference_order():
    own = lambda m: [k[len('user_encoder.'):] for k in m.state_dict()
                     if k.startswith('user_encoder.') and not k.startswith('user_encoder.news_encoder.')]
    caa = ['candidate_aware_attn.' + k for k in ('query_proj.weight', 'query_proj.bias', 'key_proj.weight', 'key_proj.bias', 'value_proj.weight',
                                                 'value_proj.bias', 'gate_proj.weight', 'gate_proj.bias', 'layernorm.weight', 'layernorm.bias')]
    att = ['attention.affine1.weight', 'attention.affine1.bias', 'attention.affine2.weight']
    assert own(Model(make_config(content_encoder='NAML', user_encoder='ATT', vocabulary_size=500))) == att + caa
    mha = ['multiheadAttention.%s.%s' % (w, p) for w in ('W_Q', 'W_K', 'W_V') for p in ('weight', 'bias')]
    assert own(Model(make_config(content_encoder='MHSA', user_encoder='MHSA', vocabulary_size=500))) == mha + ['affine.weight', 'affine.bias'] + att + caa


@pytest.mark.parametrize('name', ['user_att_naml', 'user_mhsa_mhsa', 'user_att_crown', 'user_mhsa_no_cand_aware'])
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = user_cases.build_case(name)
    sd = synth_state_dict(json.loads(str(load_golden(name)['state_dict_spec'])))
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    ue = model.user_encoder
    assert torch.equal(ue.attention.affine2.weight, sd['user_encoder.attention.affine2.weight'])
    if cfg.user_encoder == 'MHSA':
        assert torch.equal(ue.affine.weight, sd['user_encoder.affine.weight'])
        assert torch.equal(ue.multiheadAttention.W_K.bias, sd['user_encoder.multiheadAttention.W_K.bias'])


@pytest.mark.parametrize('name', user_cases.GRAD_CASES + golden_cases.ABLATION_GRAD_CASES)
def test_dead_parameters_are_the_ones_the_reference_gives_no_gradient(name):
    # the ATT / MHSA cases, and the CROWN user encoder with each switch of config.py:60-66 off (tests/golden_cases.py)
    cfg, _, _ = (user_cases if name in user_cases.CASES else golden_cases).build_case(name)
    g = load_golden('grad_' + name)
    model = Model(cfg)
    # without_grad lists every parameter whose .grad stayed None: the frozen tables (requires_grad False) and the dead ones
    frozen = [k for k, p in dict(model.named_parameters()).items() if not p.requires_grad and k in json.loads(str(g['without_grad']))]
    assert sorted(training.dead_parameters(model) + frozen) == sorted(json.loads(str(g['without_grad'])))
    assert not set(training.dead_parameters(model)) & set(frozen)
    live = [n for n in training.TrainStep.bucket_names(model)]
    assert live == json.loads(str(g['with_grad']))                     # the bucket: the reference's gradients, in its order


def test_crown_dead_set_is_what_the_substrings_select():
    cfg, _, _ = golden_cases.build_case('cfg1_crown')
    model = Model(cfg)
    want, seen = [], set()
    for n, p in model.named_parameters():
        if p.requires_grad and id(p) not in seen and any(d in n for d in training._DEAD):
            want.append(n)
        seen.add(id(p))
    assert training.dead_parameters(model) == want and len(want) > 0
    frozen = [k for k in json.loads(str(load_golden('grad_cfg1_crown')['without_grad'])) if not dict(model.named_parameters())[k].requires_grad]
    assert sorted(want + frozen) == sorted(json.loads(str(load_golden('grad_cfg1_crown')['without_grad'])))
    assert training.TrainStep.bucket_names(model) == json.loads(str(load_golden('grad_cfg1_crown')['with_grad']))


def test_mhsa_user_refuses_another_history_length():
    model = Model(make_config(content_encoder='MHSA', user_encoder='MHSA', max_history_num=10, vocabulary_size=500))
    model.user_encoder.check_history_length(10)
    with pytest.raises(ValueError, match='max_history_num = 10'):
        model.user_encoder.check_history_length(7)
