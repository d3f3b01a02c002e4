"""The baseline models -- a content encoder as the news encoder itself, no LIME (config.news_encoder = 'CROWN', 'CNN', 'NAML', 'MHSA',
'KCNN'; reference model.py:41-62) -- on the CPU: every supported pairing builds under the reference's model_name, the state_dict is
the reference's key for key and shape for shape (tests/golden/plain_*.npz, tools/make_plain_goldens.py), a reference-layout checkpoint
loads strictly, the parameters the training step leaves out are exactly the ones the reference's backward leaves without a gradient,
the pairings outside the path are refused with their reason, and LIME models keep the state_dict they had.  No GPU."""
import json

import pytest
import torch

import golden_cases
import plain_cases
import user_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, make_config, newsEncoders, training

NEWS = ['CROWN', 'CNN', 'NAML', 'MHSA', 'KCNN']
DIM = {'CROWN': 900, 'CNN': 500, 'NAML': 400, 'MHSA': 300, 'KCNN': 500}      # config.py defaults: the encoder's own width


# ATT and MHSA pair with all five; the CROWN user encoder with CROWN's own news encoder alone (test_crown_user_needs_the_crown_news_encoder)
PAIRINGS = [(n, u) for n in NEWS for u in ('ATT', 'MHSA')] + [('CROWN', 'CROWN')]


@pytest.mark.parametrize('news,user', PAIRINGS)
def test_every_supported_pairing_builds(news, user):
    # content_encoder is not read without LIME (model.py:41-62): a value no encoder has must not matter
    model = Model(make_config(news_encoder=news, user_encoder=user, content_encoder='unread', vocabulary_size=500))
    assert model.model_name == '%s-%s' % (news, user)
    assert type(model.news_encoder) is getattr(newsEncoders, news) and model.user_encoder.news_encoder is model.news_encoder
    assert model.news_embedding_dim == model.news_encoder.news_embedding_dim == DIM[news]
    keys = list(model.state_dict())
    assert 'news_encoder.word_embedding.weight' in keys
    assert not [k for k in keys if 'base_news_encoder.' in k or '.freshness_encoder.' in k or k.startswith(('news_encoder.project.', 'news_encoder.gate.'))]
    # no LIME-level category tables: the user side reads the content encoder's own, and category_embedding trains
    named = dict(model.named_parameters())
    assert named['news_encoder.category_embedding.weight'].requires_grad
    assert not named['news_encoder.subCategory_embedding.weight'].requires_grad
    model.initialize()
    assert float(model.news_encoder.subCategory_embedding.weight[0].abs().max()) == 0.0


@pytest.mark.parametrize('name', list(plain_cases.CASES))
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = plain_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))


@pytest.mark.parametrize('name', ['plain_crown_crown', 'plain_crown_att', 'plain_naml_att', 'plain_mhsa_mhsa', 'plain_cnn_mhsa', 'plain_kcnn_att',
                                  'plain_mhsa_mhsa_no_cand_aware'])
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = plain_cases.build_case(name)
    sd = synth_state_dict(json.loads(str(load_golden(name)['state_dict_spec'])))
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    assert torch.equal(model.news_encoder.word_embedding.weight, sd['news_encoder.word_embedding.weight'])
    assert torch.equal(model.news_encoder.category_embedding.weight, sd['news_encoder.category_embedding.weight'])


@pytest.mark.parametrize('name', plain_cases.GRAD_CASES)
def test_dead_parameters_are_the_ones_the_reference_gives_no_gradient(name):
    cfg, _, _ = plain_cases.build_case(name)
    g = load_golden('grad_' + name)
    model = Model(cfg)
    without = json.loads(str(g['without_grad']))
    # without_grad lists every parameter whose .grad stayed None: the frozen tables (requires_grad False) and the dead ones
    frozen = [k for k, p in dict(model.named_parameters()).items() if not p.requires_grad and k in without]
    dead = training.dead_parameters(model)
    assert sorted(dead + frozen) == sorted(without)
    assert not set(dead) & set(frozen)
    assert training.TrainStep.bucket_names(model) == json.loads(str(g['with_grad']))          # the bucket: the reference's gradients, in its order
    # the content encoder's own category_affine and the now-trainable category table are live whatever the user encoder is
    live = set(training.TrainStep.bucket_names(model))
    assert 'news_encoder.category_embedding.weight' in live
    if hasattr(model.news_encoder, 'category_affine'):
        assert 'news_encoder.category_affine.weight' in live


@pytest.mark.parametrize('name', plain_cases.GRAD_CASES)
def test_a_gradient_golden_pins_more_than_zeros(name):
    g = load_golden('grad_' + name)
    live = [k for k in json.loads(str(g['with_grad'])) if float(g['norm:' + k]) > 0.0]
    assert len(live) >= len(json.loads(str(g['with_grad']))) - 3 and float(g['loss']) > 0.0


@pytest.mark.parametrize('news', ['CNN', 'NAML', 'MHSA', 'KCNN'])
def test_crown_user_needs_the_crown_news_encoder(news):
    # userEncoders.py:103-105: news_encoder.category_affine over the 100-wide topic pair -- only CROWN's own encoder has that layer
    with pytest.raises(NotImplementedError, match='category_affine') as e:
        Model(make_config(news_encoder=news, user_encoder='CROWN', vocabulary_size=500))
    assert ('another shape' if news == 'NAML' else 'no category_affine') in str(e.value)


def test_cne_stays_refused_as_a_bare_news_encoder():
    with pytest.raises(NotImplementedError, match='per-news cache') as e:
        Model(make_config(news_encoder='CNE', user_encoder='ATT', vocabulary_size=500))
    assert "'CNE'" in str(e.value) and '1,700' in str(e.value)


@pytest.mark.parametrize('news', ['HDC', 'PNE', 'DAE', 'Inception', 'PLM_BERT', 'lime'])
def test_unknown_news_encoders_are_refused_by_name(news):
    with pytest.raises(NotImplementedError, match='CROWN, CNN, NAML, MHSA, KCNN') as e:
        Model(make_config(news_encoder=news, vocabulary_size=500))
    assert repr(news) in str(e.value)


@pytest.mark.parametrize('user', ['LSTUR', 'GRU', 'CATT'])
def test_refused_user_encoders_keep_their_message_without_lime(user):
    with pytest.raises(NotImplementedError, match='ATT, CROWN, MHSA'):
        Model(make_config(news_encoder='NAML', user_encoder=user, vocabulary_size=500))


@pytest.mark.parametrize('name', ['user_att_naml', 'user_mhsa_mhsa', 'user_att_crown', 'cfg1_crown', 'cfg1_mhsa'])
def test_lime_models_keep_their_state_dict(name):
    cfg, _, _ = (user_cases if name in user_cases.CASES else golden_cases).build_case(name)
    assert cfg.news_encoder == 'LIME'
    g = load_golden(name)
    model = Model(cfg)
    assert model.model_name == 'LIME-%s-%s' % (cfg.content_encoder, cfg.user_encoder)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))
