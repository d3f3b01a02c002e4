"""LIME-CNE-{CROWN,ATT,MHSA} (config.content_encoder = 'CNE') on the CPU: the models build, the state_dict is the reference's key for key
and shape for shape (tests/golden/cne_*.npz, tools/make_cne_goldens.py), a reference-layout checkpoint loads strictly, the gradient
bucket is the reference's set of tensors with a gradient, and what the encoder refuses is refused with a clear error.  No GPU."""
import json

import pytest
import torch

import cne_cases
from helpers import load_golden, synth_state_dict
from lime_cikm25_amd import Model, make_config, training


def _cfg(**over):
    return make_config(content_encoder='CNE', vocabulary_size=500, **over)


def test_hidden_dim_default_is_the_reference_one():
    assert make_config().hidden_dim == 400


@pytest.mark.parametrize('user', ['CROWN', 'ATT', 'MHSA'])
def test_cne_model_builds(user):
    model = Model(_cfg(user_encoder=user, hidden_dim=32))
    assert model.model_name == 'LIME-CNE-' + user
    enc = model.news_encoder.base_news_encoder
    assert enc.news_embedding_dim == 4 * 32 + 100
    assert tuple(enc.title_lstm.weight_hh_l0_reverse.shape) == (128, 32) and tuple(enc.content_lstm.weight_ih_l0.shape) == (128, 300)
    assert enc.title_H.bias is None and enc.title_M.bias is not None
    assert enc.title_cross_attention.K.bias is None and enc.title_cross_attention.Q.bias is not None


def test_default_width():
    assert Model(_cfg()).news_encoder.base_news_encoder.news_embedding_dim == 1700


@pytest.mark.parametrize('name', list(cne_cases.CASES))
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = cne_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert model.model_name == 'LIME-CNE-' + cfg.user_encoder
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(g['state_dict_spec']))


@pytest.mark.parametrize('name', ['cne_small', 'cne_att'])
def test_trainable_parameters_are_the_reference_ones(name):
    """word_embedding and CNE's re-created category_embedding train; the inherited subCategory_embedding does not (newsEncoders.py:447)."""
    cfg, _, _ = cne_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))
    enc = model.news_encoder.base_news_encoder
    assert enc.word_embedding.weight.requires_grad and enc.category_embedding.weight.requires_grad
    assert not enc.subCategory_embedding.weight.requires_grad


@pytest.mark.parametrize('name', ['cne_small', 'cne_h400_empty_history'])
def test_reference_checkpoint_loads_strictly(name):
    cfg, _, _ = cne_cases.build_case(name)
    sd = synth_state_dict(json.loads(str(load_golden(name)['state_dict_spec'])))
    model = Model(cfg)
    model.load_state_dict(sd, strict=True)
    enc = model.news_encoder.base_news_encoder
    pre = 'news_encoder.base_news_encoder.'
    for k in ('title_lstm.weight_hh_l0_reverse', 'content_lstm.bias_ih_l0', 'content_M.bias', 'title_cross_attention.K.weight',
              'content_self_attention.affine2.weight'):
        obj = enc
        for part in k.split('.'):
            obj = getattr(obj, part)
        assert torch.equal(obj, sd[pre + k]), k


@pytest.mark.parametrize('name', cne_cases.GRAD_CASES)
def test_gradient_bucket_is_the_references_set(name):
    cfg, _, _ = cne_cases.build_case(name)
    g = load_golden('grad_' + name)
    model = Model(cfg)
    with_grad, without = json.loads(str(g['with_grad'])), json.loads(str(g['without_grad']))
    frozen = {k for k, p in model.named_parameters() if not p.requires_grad}
    assert sorted(training.dead_parameters(model)) == sorted(set(without) - frozen)
    assert training.TrainStep.bucket_names(model) == with_grad
    if cfg.user_encoder == 'CROWN':
        assert len(with_grad) == 59 and len(frozen) == 3


@pytest.mark.parametrize('over,message', [(dict(compute_dtype='bf16'), 'CNE content encoder is built for fp32'),
                                          (dict(hidden_dim=24), 'multiples of 16'), (dict(hidden_dim=100), 'multiples of 16'),
                                          (dict(hidden_dim=0), 'multiples of 16')])
def test_refused_settings(over, message):
    with pytest.raises(NotImplementedError, match=message):
        Model(_cfg(**over))


@pytest.mark.parametrize('rows,news_per_row', [(64, 51), (64, 55), (32, 55), (1, 1), (1024, 150)])
def test_a_call_of_any_size_is_chunked_within_the_gi_bound(rows, news_per_row):
    """The recurrence of one encoder call runs in chunks whose gi stays within CNE.GI_BYTES_PER_PASS, at the default sizes (hidden 400,
    title 32, body 128): the reference's batch_size 64 gives 64 * 51 news in a dev pass and 64 * 55 in a [B, K] forward, more than one
    chunk holds.  The chunks cover every news once, in order; the gates pair over the whole call behind them (no size limit)."""
    enc = Model(_cfg()).news_encoder.base_news_encoder
    n = rows * news_per_row + 1
    for S in (enc.max_title_length, enc.max_content_length):
        chunks = enc.lstm_chunks(n, S)
        assert chunks[0][0] == 0 and chunks[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(r1 > r0 for r0, r1 in chunks)
        assert all((r1 - r0) * S * 8 * enc.hidden_dim * 4 <= enc.GI_BYTES_PER_PASS for r0, r1 in chunks)
    assert len(enc.lstm_chunks(64 * 55 + 1, 128)) == 2 and len(enc.lstm_chunks(64 * 55 + 1, 32)) == 1


def test_holders_are_not_a_fallback():
    enc = Model(_cfg(hidden_dim=16)).news_encoder.base_news_encoder
    x = torch.zeros(1, 4, 300)
    for holder, arg in ((enc.title_lstm, x), (enc.content_lstm, x), (enc.title_H, torch.zeros(1, 32)), (enc.content_M, torch.zeros(1, 32)),
                        (enc.title_cross_attention, torch.zeros(1, 4, 32))):
        with pytest.raises(NotImplementedError):
            holder(arg)


def test_body_mask_is_required():
    """CNE never guesses the body mask from the ids: the scoring and the training entry both raise before any kernel runs."""
    enc = Model(_cfg(hidden_dim=16)).news_encoder.base_news_encoder.eval()
    ids_t, ids_b = torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 16, dtype=torch.int32)
    mask = torch.ones(2, 8, dtype=torch.bool)
    cat = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError, match='body mask'):
        enc.encode_flat(ids_t, mask, ids_b, cat, cat, torch.empty(2, enc.news_embedding_dim))
    with pytest.raises(TypeError, match='body mask'):
        training.content_flat(enc, ids_t, mask, ids_b, cat, cat)
