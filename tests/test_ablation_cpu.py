"""The four ablation switches of the scoring path (config.py:60-66) under the CROWN user encoder, on the CPU: the state_dict of every
switch-off case is the reference's, the optimizer bucket is exactly what the reference's backward gives a gradient (the gradient goldens
of tests/golden_cases.ABLATION_GRAD_CASES, tools/make_grad_goldens.py), and the per-device constants a captured HIP graph holds by
address outlive a regrow.  No GPU."""
import gc
import json
import weakref

import pytest
import torch

import golden_cases
from helpers import load_golden
from lime_cikm25_amd import Model, newsEncoders, training

ABLATION_CASES = golden_cases.ABLATION_GRAD_CASES + ('no_residual_eval',)


@pytest.mark.parametrize('name', ABLATION_CASES)
def test_state_dict_is_the_reference_one(name):
    cfg, _, _ = golden_cases.build_case(name)
    g = load_golden(name)
    model = Model(cfg)
    spec = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert spec == json.loads(str(g['state_dict_spec']))
    assert len(spec) == (183 if cfg.use_candidate_ware_clicked_news_attention else 173)
    assert sorted(k for k, p in model.named_parameters() if p.requires_grad) == sorted(json.loads(str(g['trainable'])))


@pytest.mark.parametrize('name', golden_cases.ABLATION_GRAD_CASES)
def test_switches_move_the_right_parameters_out_of_the_bucket(name):
    """Which names a switch moves (that the dead set and the bucket ARE the reference's lists is checked for these cases by
    tests/test_user_encoders_cpu.py::test_dead_parameters_are_the_ones_the_reference_gives_no_gradient)."""
    cfg, _, _ = golden_cases.build_case(name)
    model = Model(cfg)
    dead, bucket = training.dead_parameters(model), training.TrainStep.bucket_names(model)
    gate_ln = [k for k in dict(model.named_parameters()) if 'candidate_aware_attn.gate_proj.' in k or 'candidate_aware_attn.layernorm.' in k]
    if name == 'no_residual':                                        # layers.py:84: constructed, never used
        assert len(gate_ln) == 4 and set(gate_ln) <= set(dead) and len(bucket) == 59
    # LIME's category_affine feeds the candidate-aware attention alone (userEncoders.py:103-105); the content encoder's own is live
    assert ('news_encoder.category_affine.weight' in dead) == (not cfg.use_candidate_ware_clicked_news_attention)
    assert 'news_encoder.base_news_encoder.category_affine.weight' in bucket


def _outlives_a_regrow(fn, small, large, want):
    dev = torch.device('cpu')
    first = fn(small, dev)
    ptr = first.data_ptr()
    ref = weakref.ref(first.untyped_storage())
    del first
    gc.collect()
    grown = fn(large, dev)
    assert grown.numel() == large
    gc.collect()
    storage = ref()
    assert storage is not None, 'the tensor a captured graph may hold by address was released by the regrow'
    assert storage.data_ptr() == ptr
    kept = torch.empty(0, dtype=torch.int32).set_(storage, 0, (small,))
    assert torch.equal(kept, want(small))
    assert torch.equal(grown, want(large))
    again = fn(small, dev)                                           # later callers share the newest generation
    assert again.data_ptr() == grown.data_ptr() and torch.equal(again, want(small))


def test_identity_rows_outlive_a_regrow():
    """A HIP graph captured with num_layers = 2 has the identity map's address in its token_attention_rows launches: a later caller
    that needs more rows must not release (and so let the allocator reuse) what an earlier caller was handed."""
    _outlives_a_regrow(newsEncoders._identity_rows, 100, 100000, lambda n: torch.arange(n, dtype=torch.int32))


def test_zero_ids_outlive_a_regrow():
    _outlives_a_regrow(newsEncoders._zero_ids, 100, 100000, lambda n: torch.zeros(n, dtype=torch.int32))


def test_regrow_at_least_doubles():
    """The generations kept alive are bounded by the newest one: each is at least twice the one before."""
    cache = {}
    make = lambda size: torch.zeros(size, dtype=torch.int32)
    dev = torch.device('cpu')
    for n in (10, 17, 18, 40, 41):
        assert newsEncoders._grown(cache, n, dev, 16, make).numel() == n
    sizes = [t.numel() for t in cache[('cpu', None)]]
    assert sizes == [16, 32, 64]
