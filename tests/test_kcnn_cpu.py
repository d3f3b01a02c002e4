"""LIME-KCNN-{CROWN,ATT,MHSA} (config.content_encoder = 'KCNN') on the CPU: every pairing builds, the state_dict is the reference's key for
key and shape for shape (tests/golden/kcnn_*.npz, tools/make_kcnn_goldens.py), a reference-layout checkpoint loads strictly, the
parameters the training step leaves out are exactly the ones the reference's backward leaves without a gradient, the weight packing is
the Conv2d layout, and the settings outside the encoder are refused with a clear error.  No GPU."""
import json

import pytest
import torch

import kcnn_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, layers, make_config, ops, training


def _cfg(**over):
    return make_config(content_encoder='KCNN', vocabulary_size=500, entity_size=80, **over)


def test_config_defaults_are_the_reference_ones():
    cfg = make_config()
    assert (cfg.entity_embedding_dim, cfg.context_embedding_dim) == (100, 100)                 # config.py:84-85
    assert cfg.entity_size > 0


@pytest.mark.parametrize('user', ['CROWN', 'ATT', 'MHSA'])
@pytest.mark.parametrize('over', [dict(), dict(cnn_window_size=2), dict(cnn_window_size=5), dict(cnn_method='group3', cnn_kernel_num=300),
                                  dict(cnn_method='group4')], ids=['naive', 'w2', 'w5', 'group3', 'group4'])
def test_every_pairing_builds(user, over):
    model = Model(_cfg(user_encoder=user, **over))
    assert model.model_name == 'LIME-KCNN-%s' % user
    assert model.reads_title_entity and not model.reads_content_mask
    assert 5 in model._used and 19 in model._used and (19, 5) in model._pairs
    enc = model.news_encoder.base_news_encoder
    assert enc.news_embedding_dim == model.config.cnn_kernel_num + 100
    assert enc.entity_embedding.weight.requires_grad and enc.context_embedding.weight.requires_grad
    assert tuple(enc.entity_embedding.weight.shape) == (80, 100)


def test_other_models_do_not_read_the_entity_ids():
    model = Model(make_config(content_encoder='CNN', vocabulary_size=500))
    assert not model.reads_title_entity and 5 not in model._used and 19 not in model._used


@pytest.mark.parametrize('over,exc', [
    (dict(cnn_method='group5', cnn_kernel_num=400), NotImplementedError),  # layers.py:141 asserts against it
    (dict(cnn_method='group3'), ValueError),                              # 400 % 3 != 0 (layers.py:149)
    (dict(cnn_method='group4', cnn_kernel_num=402), ValueError),          # layers.py:154
    (dict(cnn_method='group3', cnn_kernel_num=30), NotImplementedError),  # 10 outputs per conv: not a multiple of 4
    (dict(cnn_method='group4', cnn_kernel_num=40), NotImplementedError),
    (dict(cnn_kernel_num=402), NotImplementedError),
    (dict(cnn_method='nope'), ValueError),
    (dict(cnn_window_size=0), ValueError),
    (dict(cnn_window_size=5, max_title_length=4), ValueError),            # no position left to pool
    (dict(cnn_method='group4', max_title_length=3), ValueError),
    (dict(compute_dtype='bf16'), NotImplementedError),                    # the KCNN encoder is fp32 only, as CNN
])
def test_refused_settings(over, exc):
    with pytest.raises(exc):
        Model(_cfg(**over))


def test_the_pooled_positions_are_the_reference_ones():
    """layers.py:147,168-170 ('naive': T - w + 1 positions) and :150-158,172-189 (the groups: T, T - 1, T - 2, T - 3)."""
    T = 16
    spec = lambda holder: [(col, w, p, P) for _, col, w, p, P in holder.convs(T)]
    assert spec(layers.Conv2D_Pool('naive', 300, 400, 3, 3)) == [(0, 3, 1, 14)]
    assert spec(layers.Conv2D_Pool('naive', 300, 400, 2, 3)) == [(0, 2, 0, 15)]
    assert spec(layers.Conv2D_Pool('naive', 300, 400, 5, 3)) == [(0, 5, 2, 12)]
    assert spec(layers.Conv2D_Pool('group3', 300, 300, 3, 3)) == [(0, 1, 0, 16), (100, 2, 0, 15), (200, 3, 1, 14)]
    assert spec(layers.Conv2D_Pool('group4', 300, 400, 3, 3)) == [(0, 1, 0, 16), (100, 2, 0, 15), (200, 3, 1, 14), (300, 4, 1, 13)]
    with pytest.raises(NotImplementedError):
        layers.Conv2D_Pool('naive', 300, 400, 3, 3)(torch.zeros(1, 300, 8, 3))          # a parameter holder, not a fallback


@pytest.mark.parametrize('name', list(kcnn_cases.CASES))
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = kcnn_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))


@pytest.mark.parametrize('name', ['kcnn_naive', 'kcnn_w2', 'kcnn_group3', 'kcnn_group4_att', 'kcnn_mhsa'])
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = kcnn_cases.build_case(name)
    sd = synth_state_dict(json.loads(str(load_golden(name)['state_dict_spec'])))
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    enc = model.news_encoder.base_news_encoder
    prefix = 'news_encoder.base_news_encoder.'
    assert torch.equal(enc.entity_embedding.weight, sd[prefix + 'entity_embedding.weight'])
    assert torch.equal(enc.M_context.weight, sd[prefix + 'M_context.weight'])
    for conv, _, w, _, _ in enc.knowledge_cnn.convs(cfg.max_title_length):
        assert tuple(conv.weight.shape) == (conv.out_channels, cfg.word_embedding_dim, w, 3)
    first = 'conv' if cfg.cnn_method == 'naive' else 'conv1'
    assert torch.equal(getattr(enc.knowledge_cnn, first).weight, sd[prefix + 'knowledge_cnn.%s.weight' % first])


@pytest.mark.parametrize('name', kcnn_cases.GRAD_CASES)
def test_dead_and_trainable_sets_are_the_reference_ones(name):
    cfg, _, _ = kcnn_cases.build_case(name)
    g = load_golden('grad_' + name)
    model = Model(cfg)
    # without_grad lists every parameter whose .grad stayed None: the frozen tables (requires_grad False) and the dead ones
    without = json.loads(str(g['without_grad']))
    frozen = [k for k, p in dict(model.named_parameters()).items() if not p.requires_grad and k in without]
    assert sorted(training.dead_parameters(model) + frozen) == sorted(without)
    assert not set(training.dead_parameters(model)) & set(frozen)
    assert training.TrainStep.bucket_names(model) == json.loads(str(g['with_grad']))       # the bucket: the reference's gradients, in its order
    prefix = 'news_encoder.base_news_encoder.'
    for k in ('entity_embedding.weight', 'context_embedding.weight', 'M_entity.weight', 'M_entity.bias', 'M_context.weight', 'M_context.bias',
              'word_embedding.weight', 'category_embedding.weight'):
        assert prefix + k in training.TrainStep.bucket_names(model)


def test_conv_pool_pack_is_the_conv2d_layout():
    """Column (src * window + j) * C + c of row o holds weight[o, c, j, src]."""
    g = torch.Generator().manual_seed(3)
    w = torch.rand(8, 12, 4, 3, generator=g)
    packed = ops.conv_pool_pack(w)
    assert tuple(packed.shape) == (8, 3 * 4 * 12) and packed.is_contiguous()
    assert torch.equal(packed, torch.einsum('ocjs->osjc', w).reshape(8, -1))
    assert float(packed[5, (2 * 4 + 1) * 12 + 7]) == float(w[5, 7, 1, 2])
    # the unfused form's per-source operands: an even window is the next odd one behind a zero first tap
    assert ops.conv_pool_odd_window(1, 0) == (1, 0) and ops.conv_pool_odd_window(3, 1) == (3, 0) and ops.conv_pool_odd_window(5, 2) == (5, 0)
    assert ops.conv_pool_odd_window(2, 0) == (3, 1) and ops.conv_pool_odd_window(4, 1) == (5, 1)
    per, wodd = ops.conv_pool_unfused_weights(packed, 3, 4, 1, 12)
    assert wodd == 5 and len(per) == 3
    for s in range(3):
        v = per[s].view(8, 5, 12)
        assert torch.all(v[:, 0] == 0) and torch.equal(v[:, 1:], w[:, :, :, s].permute(0, 2, 1))


def test_the_entity_ids_are_never_guessed():
    model = Model(_cfg())
    enc = model.news_encoder.base_news_encoder
    ids = torch.zeros(2, 32, dtype=torch.int32)
    with pytest.raises(TypeError, match='title_entity'):
        enc.encode_flat(ids, ids.bool(), ids, ids[:, 0], ids[:, 0], torch.zeros(2, 500))
    with pytest.raises(TypeError, match='title_entity'):
        model.eval().score_impressions(*([torch.zeros(1, 2, 3)] * 8 + [torch.zeros(1, 2)] * 8))
