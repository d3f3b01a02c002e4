"""LIME-CNN-CROWN (config.content_encoder = 'CNN') on the CPU: the settings the reference refuses or fails on are refused with a
clear error, the state_dict is the reference's key for key and shape for shape (tests/golden/cnn_*.npz, tools/make_cnn_goldens.py),
and a reference-layout checkpoint loads strictly.  No GPU."""
import json

import pytest
import torch

import cnn_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, make_config


def _cfg(**over):
    return make_config(content_encoder='CNN', vocabulary_size=500, **over)


def test_config_defaults_are_the_reference_ones():
    cfg = make_config()
    assert (cfg.cnn_method, cfg.cnn_kernel_num, cfg.cnn_window_size) == ('naive', 400, 3)       # config.py:86-88


@pytest.mark.parametrize('over,exc', [
    (dict(cnn_method='group4'), ValueError),                              # layers.py:100 asserts against it
    (dict(cnn_method='group5', cnn_kernel_num=400), NotImplementedError),  # layers.py:131-134 fails on shape
    (dict(cnn_window_size=4), ValueError),                                # output T - 1 long
    (dict(cnn_window_size=2), ValueError),
    (dict(cnn_method='group3'), ValueError),                              # 400 % 3 != 0 (layers.py:105)
    (dict(cnn_method='group3', cnn_kernel_num=301), ValueError),
    (dict(cnn_method='group3', cnn_kernel_num=30), NotImplementedError),  # 10 outputs per conv: not a multiple of 4
    (dict(compute_dtype='bf16'), NotImplementedError),                    # the CNN encoder is fp32 only
])
def test_refused_settings(over, exc):
    with pytest.raises(exc):
        Model(_cfg(**over))


@pytest.mark.parametrize('name', ['cnn_naive', 'cnn_group3', 'cnn_w5_full_len'])
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = cnn_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert model.model_name == 'LIME-CNN-CROWN'
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))


def test_trainable_parameters_are_the_reference_ones():
    """word_embedding and the CNN's re-created category_embedding train; subCategory_embedding does not (newsEncoders.py:540-541)."""
    cfg, _, _ = cnn_cases.build_case('cnn_naive')
    g = load_golden('cnn_naive')
    model = Model(cfg)
    got = sorted(k for k, p in model.named_parameters() if p.requires_grad)
    assert got == sorted(json.loads(str(g['trainable'])))
    enc = model.news_encoder.base_news_encoder
    assert enc.word_embedding.weight.requires_grad and enc.category_embedding.weight.requires_grad
    assert not enc.subCategory_embedding.weight.requires_grad


@pytest.mark.parametrize('name', ['cnn_naive', 'cnn_group3'])
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = cnn_cases.build_case(name)
    spec = json.loads(str(load_golden(name)['state_dict_spec']))
    sd = synth_state_dict(spec)
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    conv = model.news_encoder.base_news_encoder.conv
    if cfg.cnn_method == 'naive':
        assert torch.equal(conv.conv.weight, sd['news_encoder.base_news_encoder.conv.conv.weight'])
        assert tuple(conv.conv.weight.shape) == (cfg.cnn_kernel_num, cfg.word_embedding_dim, cfg.cnn_window_size)
    else:
        assert [c.kernel_size[0] for c, _ in conv.convs()] == [1, 3, 5]
        assert [col for _, col in conv.convs()] == [0, 100, 200]


def test_conv_holder_forward_is_not_a_fallback():
    cfg = _cfg()
    model = Model(cfg)
    with pytest.raises(NotImplementedError):
        model.news_encoder.base_news_encoder.conv(torch.zeros(1, cfg.word_embedding_dim, 8))
