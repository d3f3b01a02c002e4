"""The staleness rule of newsEncoders.WeightProducts (kept.weight_state / weight_state_stale: pure host functions) and the binding of the
attention entry that reads the products.  CPU only."""
import ctypes

import torch
import torch.nn as nn

from lime_cikm25_amd import _lib, kept, newsEncoders, ops


def _state(sources, writes=0):
    return kept.weight_state(sources, writes)


def test_staleness_rule():
    lin = nn.Linear(6, 4)
    table = torch.zeros(5, 6)
    src = [table, lin.weight, lin.bias]
    assert kept.weight_state_stale(None, _state(src)) == 'never'
    rec = _state(src)
    assert kept.weight_state_stale(rec, _state(src)) is None
    with torch.no_grad():
        lin.weight.mul_(2.0)                                       # an in-place op under no_grad
    assert kept.weight_state_stale(rec, _state(src)) == 'version'
    rec = _state(src)
    lin.load_state_dict({'weight': torch.ones(4, 6), 'bias': torch.ones(4)})
    assert kept.weight_state_stale(rec, _state(src)) == 'version'
    rec = _state(src)
    table.copy_(torch.ones(5, 6))
    assert kept.weight_state_stale(rec, _state(src)) == 'version'
    rec = _state(src)
    lin.weight.data.add_(1.0)                                      # the blind spot: neither version nor address moves ...
    assert kept.weight_state_stale(rec, _state(src)) is None
    assert kept.weight_state_stale(rec, _state(src, writes=1)) == 'writes'      # ... the writer counter does
    lin.weight.data = torch.zeros(4, 6)                            # re-pointed storage (TrainStep's flat bucket, .to())
    assert kept.weight_state_stale(rec, _state(src)) == 'moved'
    rec = _state(src)
    assert kept.weight_state_stale(rec, _state([torch.zeros(7, 6), lin.weight, lin.bias])) == 'moved'      # another shape
    assert kept.weight_state_stale(rec, _state(src[:2])) == 'moved'                                         # another source list
    assert kept.weight_state_stale(rec, _state(src)) is None


def test_state_is_host_data_only():
    t = torch.zeros(3, 4)
    (entries, writes) = kept.weight_state([t], 7)
    assert entries == ((t.data_ptr(), (3, 4), t._version),) and writes == 7


def test_writer_counter_counts():
    before = ops.PARAM_WRITES
    ops.note_param_write()
    assert ops.PARAM_WRITES == before + 1


def test_applicability_follows_the_native_entry():
    ok = newsEncoders.vocab_qkv_applicable
    assert ok(32, 300, 10) and ok(64, 300, 10) and ok(128, 300, 10)
    assert not ok(96, 300, 10) and not ok(256, 300, 10) and not ok(512, 300, 10)         # the long-sequence kernel is not covered
    assert not ok(128, 400, 10)                                                           # heads wider than 32 columns
    assert 'vocab' in _lib.ATTN_FORM
    assert _lib.SIGNATURES['lime_token_attention_f32'][1] == [ctypes.POINTER(_lib.TokenAttentionArgs), ctypes.c_void_p]
