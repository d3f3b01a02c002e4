"""The news-side tail once per distinct news (newsEncoders.NEWS_DEDUP, DESIGN.md "Distinct news behind the encoders"): Model.forward
with the switch on against the switch off -- the same kernels and the same arithmetic for every computed row, so the logits are
compared bit for bit -- eagerly, through one captured graph replayed under other device counts, and with the token-level DEDUP off
(where the switch must have no effect)."""
import numpy as np
import pytest
import torch

from lime_cikm25_amd import make_config, newsEncoders, ops, synth
from test_model_gpu import gpu_model, run

pytestmark = pytest.mark.gpu

HIST_KEYS = ('user_category', 'user_subCategory', 'user_freshness', 'user_user_topic_lifetime')


def _with_history(cfg, batch, n_keep):
    """A copy of ``batch`` whose impressions all keep ``n_keep`` history slots: slots in front of it that were padding get fresh texts
    (their keys stay the padding news' zeros: live through their texts alone), the slots from it on become the padding news of
    synth.make_batch -- all-zero texts, mask bit 0 set, category / subCategory / freshness / lifetime 0."""
    rng = np.random.default_rng(11)
    b2 = {k: v.clone() for k, v in batch.items()}
    B, H = b2['user_history_mask'].shape
    for key, S in (('user_title_text', cfg.max_title_length), ('user_content_text', cfg.max_abstract_length)):
        t = b2[key]
        t[:, n_keep:] = 0
        for b in range(B):
            for h in range(n_keep):
                if not bool((t[b, h] != 0).any()):
                    ln = int(rng.integers(3, S + 1))
                    t[b, h, :ln] = torch.from_numpy(rng.integers(1, cfg.vocabulary_size, size=ln).astype(np.int32))
    for key, text in (('user_title_mask', 'user_title_text'), ('user_content_mask', 'user_content_text')):
        b2[key] = b2[text] != 0
        b2[key][..., 0] = True
    for key in HIST_KEYS:
        b2[key][:, n_keep:] = 0
    b2['user_history_mask'][:, :n_keep] = True
    b2['user_history_mask'][:, n_keep:] = False
    return b2


@pytest.fixture(scope='module')
def setup():
    cfg = make_config(batch_size=8, max_history_num=30, max_title_length=32, max_abstract_length=64)
    model, _ = gpu_model(cfg, seed=71)
    A = synth.make_batch(cfg, 8, 2, seed=72)
    batches = {'A': A, 'full': _with_history(cfg, A, cfg.max_history_num), 'empty': _with_history(cfg, A, 0),
               'large': synth.make_batch(cfg, 12, 2, seed=73)}
    # the yardstick, computed once: the switch off (every slot through the tail), eagerly
    old = (newsEncoders.NEWS_DEDUP, newsEncoders.DEDUP, model.use_graph)
    newsEncoders.NEWS_DEDUP, newsEncoders.DEDUP, model.use_graph = False, True, False
    try:
        want = {name: run(model, b, False) for name, b in batches.items()}
    finally:
        newsEncoders.NEWS_DEDUP, newsEncoders.DEDUP, model.use_graph = old
    yield cfg, model, batches, want
    model._graphs.clear()


def _took_the_path(model, cfg, batch):
    """The batch is on the path under test: M = B (N + H) = 256 news, (M + 1) S >= 4096 rows for both encoders."""
    enc = model.news_encoder.base_news_encoder
    M = batch['news_category'].numel() + batch['user_category'].numel()
    t = torch.zeros((M, cfg.max_title_length), dtype=torch.int32, device='cuda')
    b = torch.zeros((M, cfg.max_abstract_length), dtype=torch.int32, device='cuda')
    return M, enc.news_dedup_applicable(t, b)


@pytest.mark.parametrize('name', ['A', 'full', 'empty'])
def test_logits_with_the_switch_on_equal_those_with_it_off(setup, name, monkeypatch):
    cfg, model, batches, want = setup
    M, on_path = _took_the_path(model, cfg, batches[name])
    assert M == 256 and on_path
    monkeypatch.setattr(newsEncoders, 'DEDUP', True)
    monkeypatch.setattr(newsEncoders, 'NEWS_DEDUP', True)
    monkeypatch.setattr(model, 'use_graph', False)
    calls = []
    real = ops.compact_batch
    monkeypatch.setattr(ops, 'compact_batch', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    got = run(model, batches[name], False)
    assert calls, 'the forward did not take the distinct-news tail'
    diff = float((got - want[name]).abs().max())
    print('%s: switch on vs off, max |difference| %.3e over logits of magnitude %.3e' % (name, diff, float(want[name].abs().max())))
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want[name]), (name, diff)


def test_one_captured_graph_follows_the_news_counts(setup, monkeypatch):
    """Captured on batch A; a larger shape in between (its own graph, and buffers that grow); then the first graph replayed on the
    full and the empty histories: other live counts, other news counts, in the buffers of the capture."""
    cfg, model, batches, want = setup
    monkeypatch.setattr(newsEncoders, 'DEDUP', True)
    monkeypatch.setattr(newsEncoders, 'NEWS_DEDUP', True)
    monkeypatch.setattr(model, 'use_graph', True)
    model._graphs.clear()
    got = [(name, run(model, batches[name], False)) for name in ('A', 'large', 'full', 'empty', 'A')]
    assert len(model._graphs) == 2, 'one graph per shape: the replays at the first shape must reuse its graph'
    for name, out in got:
        diff = float((out - want[name]).abs().max())
        print('graph, batch %s: max |difference| to the switch-off logits %.3e' % (name, diff))
        assert bool(torch.isfinite(out).all()) and torch.equal(out, want[name]), (name, diff)
    model._graphs.clear()


def test_without_token_dedup_the_switch_has_no_effect(setup, monkeypatch):
    cfg, model, batches, want = setup
    monkeypatch.setattr(newsEncoders, 'DEDUP', False)
    monkeypatch.setattr(model, 'use_graph', False)
    calls = []
    real = ops.compact_batch
    monkeypatch.setattr(ops, 'compact_batch', lambda *a, **kw: calls.append(1) or real(*a, **kw))
    outs = []
    for switch in (True, False):
        monkeypatch.setattr(newsEncoders, 'NEWS_DEDUP', switch)
        outs.append(run(model, batches['A'], False))
    assert not calls and torch.equal(outs[0], outs[1])
