"""The model with out_proj + norm1 on lime_encoder_oproj_sp (newsEncoders._oproj_sp_applicable) against the same model with the
switch off (lime_linear_f32's fp32 kernel) and against the oracle, at the config-2 shape with a 3000-word table; and the packed
out_proj weight of newsEncoders.WeightProducts under a captured graph: refreshed in place when the weight changes."""
import pytest
import torch

from helpers import rel_err
from lime_cikm25_amd import make_config, newsEncoders, ops, synth
from lime_cikm25_amd.training import TrainStep
from oracle import lime_oracle as O
from test_model_gpu import gpu_model, run
from test_vocab_qkv_gpu import _batch, _products

pytestmark = pytest.mark.gpu


def _launches(model, batch, monkeypatch):
    """Kernel names of one eager forward under the per-launch profile."""
    prof = []
    monkeypatch.setattr(ops, 'PROFILE', prof)
    monkeypatch.setattr(model, 'use_graph', False)
    run(model, batch, False)
    monkeypatch.setattr(ops, 'PROFILE', None)
    monkeypatch.setattr(model, 'use_graph', True)
    return [rec[0] for rec in prof]


@pytest.mark.parametrize('mode', ['mind_shaped', 'no_padding', 'only_padding'])
def test_model_with_the_switch_on_and_off(mode, monkeypatch):
    """Both sides carry fp32-level products: the path-to-path bound of tests/test_vocab_qkv_gpu.py, and its oracle bound."""
    cfg = make_config(vocabulary_size=3000)
    model, sd = gpu_model(cfg, seed=23)
    batch = _batch(cfg, mode)
    monkeypatch.setattr(newsEncoders, 'SP_OPROJ', True)
    got = run(model, batch, False)
    names = _launches(model, batch, monkeypatch)
    assert names.count('oproj_sp_kernel') == 2, names                # title and body took the launch
    wp = _products(model)
    assert wp is not None and all(e['oproj'][0] is not None for e in wp.encoder)
    monkeypatch.setattr(newsEncoders, 'SP_OPROJ', False)
    model._graphs.clear()
    off = run(model, batch, False)
    assert 'oproj_sp_kernel' not in _launches(model, batch, monkeypatch)
    model._graphs.clear()
    e = rel_err(got.numpy(), off.numpy())
    print('%s: switch on vs off %.2e' % (mode, e))
    assert torch.isfinite(got).all() and e < 2e-6
    if mode == 'mind_shaped':
        e_oracle = rel_err(got.numpy(), O.model_forward(sd, cfg, batch).numpy())
        print('%s: switch on vs oracle %.2e' % (mode, e_oracle))
        assert e_oracle < 1e-3


def test_dense_route_takes_the_launch(monkeypatch):
    """Without the compaction (the dense fp32 scoring route) the rule holds as well: both sides of the dense-versus-compacted
    comparisons keep one kernel family."""
    cfg = make_config(vocabulary_size=3000)
    model, _ = gpu_model(cfg, seed=23)
    batch = _batch(cfg, 'mind_shaped')
    monkeypatch.setattr(newsEncoders, 'SP_OPROJ', True)
    compacted = run(model, batch, False)
    monkeypatch.setattr(newsEncoders, 'DEDUP', False)
    model._graphs.clear()
    dense = run(model, batch, False)
    assert _launches(model, batch, monkeypatch).count('oproj_sp_kernel') == 2
    model._graphs.clear()
    e = rel_err(dense.numpy(), compacted.numpy())
    print('dense vs compacted, switch on: %.2e' % e)
    assert e < 2e-6


def test_packed_out_proj_is_refreshed_in_place_under_the_captured_graph(monkeypatch):
    cfg = make_config(vocabulary_size=3000)
    model, _ = gpu_model(cfg, seed=23)
    monkeypatch.setattr(newsEncoders, 'SP_OPROJ', True)
    model.eval()
    ts = TrainStep(model, lr=1e-3, gradient_clip_norm=4.0)         # (re-points the parameters and drops the graphs: before the first capture)
    batch = _batch(cfg, 'mind_shaped')
    enc = model.news_encoder.base_news_encoder
    last = run(model, batch, False)
    packs = lambda: [p.data_ptr() for e in _products(model).encoder for p in e['oproj']]
    ptrs, refreshes = packs(), _products(model).refreshes
    assert len(model._graphs) == 1 and len(ptrs) == 2
    graph = next(iter(model._graphs.values()))[0]

    def eager(switch):
        monkeypatch.setattr(newsEncoders, 'SP_OPROJ', switch)
        model.use_graph = False
        try:
            return run(model, batch, False)
        finally:
            model.use_graph = True
            monkeypatch.setattr(newsEncoders, 'SP_OPROJ', True)

    def check(what, bound):
        """The replay computes what an eager forward over the same kernels computes, bit for bit (a stale pack, or a fresh one at
        another address, cannot); against the switch-off forward, which reads Wo itself, only the paths' fp32-level difference is
        left, where a stale pack would leave the whole move of the logits."""
        nonlocal last, refreshes
        got = run(model, batch, False)                             # a replay of the first capture
        assert _products(model).refreshes == refreshes + 1, what   # (the replay refreshed them, not the eager forwards below)
        e = rel_err(got.numpy(), eager(False).numpy())
        print('%s: replay vs switch-off forward %.2e, moved %.2e' % (what, e, rel_err(got.numpy(), last.numpy())))
        assert torch.equal(got, eager(True)), what
        assert e < bound, what
        assert rel_err(got.numpy(), last.numpy()) > 1e-4, what     # the logits followed the weights
        assert len(model._graphs) == 1 and next(iter(model._graphs.values()))[0] is graph and packs() == ptrs, what
        assert _products(model).refreshes == refreshes + 1, what
        last, refreshes = got, _products(model).refreshes

    train = [v.cuda() for v in synth.make_batch(cfg, 4, 3, seed=5).values()]
    model.train()
    for _ in range(3):
        ts.step(*train)                                            # the native Adam writes the flat bucket through its address
    model.eval()
    check('TrainStep.step', 2e-6)                                  # the path-to-path bound of tests/test_vocab_qkv_gpu.py
    with torch.no_grad():
        enc.body_transformer.layers[0].self_attn.out_proj.weight.mul_(1.5)     # Wo alone: it is one of the products' sources
    # the two paths differ in the rounding of the attn Wo^T product alone, and that product is now 1.5 times as large beside an
    # unchanged residual: 1.5 times the path-to-path bound (measured: 3.2e-7 here, 2.6e-6 with this edit on the initial weights)
    check('in-place op on out_proj.weight', 1.5 * 2e-6)
    again = run(model, batch, False)                               # nothing changed: nothing recomputed
    assert torch.equal(again, last) and _products(model).refreshes == refreshes
