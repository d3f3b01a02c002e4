"""The weight-only preparation kept across scoring forwards (newsEncoders.WEIGHT_PREP_CACHE): CROWN's stacked intent weights in
``WeightProducts`` and LIME's ``OccurrenceTables``.  Kept or recomputed, the same kernels compute the same values, so every comparison
is bit for bit: the switch on against off, a model whose weights changed under its captured graph against a freshly built model with the
same weights (the graph itself must survive: nothing moved), the 'gated' and 'add' fusions, and the cache stepping aside under
autograd."""
import pytest
import torch

from lime_cikm25_amd import Model, make_config, newsEncoders, synth
from test_model_gpu import gpu_model, run

pytestmark = pytest.mark.gpu


def _cfg(**kw):
    return make_config(batch_size=8, max_history_num=30, max_title_length=32, max_abstract_length=64, vocabulary_size=3000, **kw)


@pytest.fixture(scope='module')
def setup():
    cfg = _cfg()
    model, _ = gpu_model(cfg, seed=71)
    batch = synth.make_batch(cfg, 8, 2, seed=72)
    yield cfg, model, batch
    model._graphs.clear()


def _fresh_logits(cfg, model, batch):
    """A newly built model holding ``model``'s weights as they are now: nothing kept, nothing captured."""
    other = Model(cfg)
    other.load_state_dict({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    other = other.cuda()
    other.use_graph = False
    return run(other, batch, False)


def test_switch_on_equals_switch_off_eagerly_and_through_the_graph(setup, monkeypatch):
    cfg, model, batch = setup
    ne, enc = model.news_encoder, model.news_encoder.base_news_encoder
    out = {}
    for on in (True, False):
        monkeypatch.setattr(newsEncoders, 'WEIGHT_PREP_CACHE', on)
        for graph in (False, True):
            monkeypatch.setattr(model, 'use_graph', graph)
            model._graphs.clear()
            out[on, graph] = run(model, batch, False)
            if graph:
                assert len(model._graphs) == 1
            if on:
                assert enc._products.intent and ne._tables is not None and ne._tables.T is not None
            else:
                assert not enc._products.intent
    model._graphs.clear()
    assert bool(torch.isfinite(out[True, True]).all())
    for key, got in out.items():
        assert torch.equal(got, out[False, False]), key


def _add(t, x):
    with torch.no_grad():
        t.add_(x)


def _mutate(model, how):
    enc, fe = model.news_encoder.base_news_encoder, model.news_encoder.freshness_encoder
    if how == 'intent_bias':
        _add(enc.intent_layers[1].bias, 0.25)
    elif how == 'dense_weight':
        _add(fe.dense.weight, 0.05)
    elif how == 'data_edit':
        enc.intent_layers[0].weight.data.mul_(1.25)                  # moves neither version nor address ...
        fe.lifetime_embedding.weight.data.add_(0.1)
        model.weights_changed()                                      # ... so the caller says so
    elif how == 'load_state_dict':
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        for k in sd:
            if k.endswith('intent_layers.2.weight') or k.endswith('news_encoder.project.bias') or k.endswith('freshness_embedding.weight'):
                sd[k] = sd[k] * 1.5 + 0.01
        model.load_state_dict(sd)
    else:
        raise KeyError(how)


@pytest.mark.parametrize('how', ['intent_bias', 'dense_weight', 'data_edit', 'load_state_dict'])
def test_changed_weights_reach_the_next_replay_without_a_recapture(setup, how, monkeypatch):
    cfg, model, batch = setup
    monkeypatch.setattr(newsEncoders, 'WEIGHT_PREP_CACHE', True)
    monkeypatch.setattr(model, 'use_graph', True)
    ne, enc = model.news_encoder, model.news_encoder.base_news_encoder
    before = run(model, batch, False)
    graphs = model._graphs
    assert len(graphs) == 1
    graph = next(iter(graphs.values()))[0]
    ptrs = [enc._products.intent['w'].data_ptr(), enc._products.intent['b'].data_ptr(), ne._tables.T.data_ptr()]
    refreshes = (enc._products.refreshes, ne._tables.refreshes)
    _mutate(model, how)
    got = run(model, batch, False)
    want = _fresh_logits(cfg, model, batch)
    print('%s: moved the logits by %.3e' % (how, float((got - before).abs().max())))
    assert not torch.equal(got, before), 'the mutation must reach the logits'
    assert torch.equal(got, want), how
    # no buffer moved: the same dictionary, the same graph in it, the same kept buffers, refreshed at most once each
    assert model._graphs is graphs and len(graphs) == 1 and next(iter(graphs.values()))[0] is graph
    assert [enc._products.intent['w'].data_ptr(), enc._products.intent['b'].data_ptr(), ne._tables.T.data_ptr()] == ptrs
    now = (enc._products.refreshes, ne._tables.refreshes)
    assert all(0 <= b - a <= 1 for a, b in zip(refreshes, now)) and now != refreshes
    again = run(model, batch, False)                                 # nothing changed: nothing recomputed
    assert torch.equal(again, got) and (enc._products.refreshes, ne._tables.refreshes) == now


@pytest.mark.parametrize('fusion', ['gated', 'add'])
def test_other_fusions_take_the_kept_tables(fusion, monkeypatch):
    cfg = _cfg(fusion_method=fusion)
    model, _ = gpu_model(cfg, seed=71)
    model.use_graph = False
    batch = synth.make_batch(cfg, 8, 2, seed=72)
    ne = model.news_encoder
    # the occurrences of a news cache (LIME.encode_cached: the serving side's reader of the tables under these fusions)
    cdim = ne.base_news_encoder.news_embedding_dim
    g = torch.Generator().manual_seed(3)
    cache = (torch.rand(20, 2 * cdim if fusion == 'gated' else cdim, generator=g) - 0.5).cuda()
    idx = torch.randint(0, 20, (77,), generator=g, dtype=torch.int32).cuda()
    fr, lt = (torch.rand(77, generator=g) * 1e6).cuda(), (torch.rand(77, generator=g) * 1e7).cuda()
    monkeypatch.setattr(newsEncoders, 'WEIGHT_PREP_CACHE', False)
    with torch.no_grad():
        T0, Q0 = ne.occurrence_tables()
        occ_off = ne.encode_cached(cache, idx, fr, lt)
    off = run(model, batch, False)
    assert getattr(ne, '_tables', None) is None
    monkeypatch.setattr(newsEncoders, 'WEIGHT_PREP_CACHE', True)
    on = run(model, batch, False)
    with torch.no_grad():
        occ_on = ne.encode_cached(cache, idx, fr, lt)
        T, Q = ne.occurrence_tables()
        assert ne.occurrence_tables()[0] is T                        # kept: the same tensor from call to call
    assert torch.equal(on, off) and torch.equal(T, T0) and torch.equal(occ_on, occ_off) and bool(torch.isfinite(occ_on).all())
    assert (Q is None and Q0 is None) if fusion == 'add' else torch.equal(Q, Q0)
    assert ne._tables.refreshes == 1


def test_under_autograd_the_cache_steps_aside(setup, monkeypatch):
    """Grad mode on and sources that require grad: the call computes its own tables -- new tensors, not the kept buffers, and the holder
    is neither consulted nor refreshed.  (The tables carry no ``grad_fn`` on either path: they come out of kernels that are handed raw
    pointers, and tests/test_cached_occurrence_cpu.py pins those launches with autograd recording; the differentiable freshness path
    is training.news_flat's.)"""
    cfg, model, batch = setup
    monkeypatch.setattr(newsEncoders, 'WEIGHT_PREP_CACHE', True)
    ne = model.news_encoder
    with torch.no_grad():
        kept, _ = ne.occurrence_tables()
    assert ne._tables is not None and kept is ne._tables.T
    refreshes = ne._tables.refreshes
    assert all(p.requires_grad for p in ne._table_sources())
    with torch.enable_grad():
        assert ne._kept_tables() is None
        T, Q = ne.occurrence_tables()
        with torch.no_grad():
            ne.freshness_encoder.dense.bias.add_(0.5)                # stale now -- and nobody refreshes under autograd
        T2, _ = ne.occurrence_tables()
    assert Q is None and T is not kept and T.data_ptr() != kept.data_ptr() and T2.data_ptr() != kept.data_ptr()
    assert ne._tables.refreshes == refreshes
    assert torch.equal(T, kept) and not torch.equal(T2, kept)       # the same kernels on the same weights; then on the new ones
    with torch.no_grad():
        assert ne.occurrence_tables()[0] is kept and torch.equal(kept, T2) and ne._tables.refreshes == refreshes + 1
    for p in ne._table_sources():                                    # no source takes gradients: nothing to record, the kept tables serve
        p.requires_grad_(False)
    try:
        with torch.enable_grad():
            assert ne.occurrence_tables()[0] is kept
    finally:
        for p in ne._table_sources():
            p.requires_grad_(True)
