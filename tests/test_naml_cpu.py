"""LIME-NAML-CROWN (config.content_encoder = 'NAML') on the CPU: the model builds, the settings the reference refuses or fails on are
refused with a clear error, the state_dict is the reference's key for key and shape for shape (tests/golden/naml_*.npz,
tools/make_naml_goldens.py), and a reference-layout checkpoint loads strictly.  No GPU."""
import json

import pytest
import torch

import naml_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, make_config


def _cfg(**over):
    return make_config(content_encoder='NAML', vocabulary_size=500, **over)


def test_naml_model_builds():
    model = Model(_cfg())
    assert model.model_name == 'LIME-NAML-CROWN'
    ne = model.news_encoder
    # no feature_fusion: the content is cnn_kernel_num wide, and LIME's freshness dense / project follow it (newsEncoders.py:42-43,
    # :106-107: 'add' or 'gated' is truthy)
    assert ne.base_news_encoder.news_embedding_dim == 400
    assert tuple(ne.freshness_encoder.dense.weight.shape) == (400, 1000)
    assert tuple(ne.project.weight.shape) == (400, 800)


@pytest.mark.parametrize('over,exc', [
    (dict(cnn_method='group4'), ValueError),                              # layers.py:100 asserts against it
    (dict(cnn_method='group5', cnn_kernel_num=400), NotImplementedError),  # layers.py:131-134 fails on shape
    (dict(cnn_window_size=4), ValueError),                                # output T - 1 long
    (dict(cnn_window_size=2), ValueError),
    (dict(cnn_method='group3'), ValueError),                              # 400 % 3 != 0 (layers.py:105)
    (dict(cnn_method='group3', cnn_kernel_num=301), ValueError),
    (dict(cnn_method='group3', cnn_kernel_num=30), NotImplementedError),  # 10 outputs per conv: not a multiple of 4
    (dict(compute_dtype='bf16'), NotImplementedError),                    # the NAML encoder is fp32 only
])
def test_refused_settings(over, exc):
    with pytest.raises(exc):
        Model(_cfg(**over))


@pytest.mark.parametrize('name', ['naml_naive', 'naml_group3', 'naml_w5_body128', 'naml_empty_history', 'naml_eval'])
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = naml_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert model.model_name == 'LIME-NAML-CROWN'
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))


def test_trainable_parameters_are_the_reference_ones():
    """word_embedding and NAML's re-created category_embedding train; the inherited subCategory_embedding does not
    (newsEncoders.py:656)."""
    cfg, _, _ = naml_cases.build_case('naml_naive')
    g = load_golden('naml_naive')
    model = Model(cfg)
    got = sorted(k for k, p in model.named_parameters() if p.requires_grad)
    assert got == sorted(json.loads(str(g['trainable'])))
    enc = model.news_encoder.base_news_encoder
    assert enc.word_embedding.weight.requires_grad and enc.category_embedding.weight.requires_grad
    assert not enc.subCategory_embedding.weight.requires_grad
    assert enc.affine2.bias is None


@pytest.mark.parametrize('name', ['naml_naive', 'naml_group3'])
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = naml_cases.build_case(name)
    spec = json.loads(str(load_golden(name)['state_dict_spec']))
    sd = synth_state_dict(spec)
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    enc = model.news_encoder.base_news_encoder
    pre = 'news_encoder.base_news_encoder.'
    for conv in ('title_conv', 'content_conv'):
        holder = getattr(enc, conv)
        if cfg.cnn_method == 'naive':
            assert torch.equal(holder.conv.weight, sd[pre + conv + '.conv.weight'])
        else:
            assert [c.kernel_size[0] for c, _ in holder.convs()] == [1, 3, 5]
    assert torch.equal(enc.affine1.weight, sd[pre + 'affine1.weight'])
    assert torch.equal(enc.content_attention.affine2.weight, sd[pre + 'content_attention.affine2.weight'])
    assert torch.equal(enc.subCategory_affine.bias, sd[pre + 'subCategory_affine.bias'])


def test_conv_holders_are_not_a_fallback():
    cfg = _cfg()
    enc = Model(cfg).news_encoder.base_news_encoder
    for holder in (enc.title_conv, enc.content_conv):
        with pytest.raises(NotImplementedError):
            holder(torch.zeros(1, cfg.word_embedding_dim, 8))
