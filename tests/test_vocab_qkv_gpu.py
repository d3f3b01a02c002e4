"""The first encoder layer over a per-vocabulary in_proj product (csrc/token_attn_sp_f32.hip token_attn_sp_vocab_kernel,
newsEncoders.WeightProducts): the attention kernel bit for bit against the dense kernel over the materialised rows, the model with
the products against the in-graph in_proj, the staleness rule through a captured graph (in-place op, load_state_dict, native Adam,
``.data`` edit + ``weights_changed``), and the fall-backs bit for bit against the switch-off path."""
import math

import numpy as np
import pytest
import torch

from helpers import rel_err
from lime_cikm25_amd import make_config, newsEncoders, ops, synth
from lime_cikm25_amd.training import TrainStep
from oracle import lime_oracle as O
from test_model_gpu import gpu_model, run

pytestmark = pytest.mark.gpu

V, HD = 700, 30
# the grid is capped at 512 workgroups: every shape takes a second trip through the persistent loop, the last group partly dead
SHAPES = [(32, 207, 10), (64, 207, 5), (128, 53, 10)]               # S, n_seq, n_head: 517.5 / 517.5 / 530 groups


@pytest.fixture
def split_forced():
    prev = ops.set_split_gemm(True, force=True)        # the kernel tests: the split product whatever the dispatcher's fill rules say
    yield
    ops.set_split_gemm(prev)


_CASES = {}


def _case(S, n_seq, h):
    """EW, pew, ids (padding tails, ids 0 and V - 1 present) and the dense kernel's output over EW[ids] + pew[t]: once per shape."""
    if (S, n_seq, h) not in _CASES:
        W = h * 32
        g = torch.Generator().manual_seed(S + n_seq)
        ew = torch.rand(V, 3 * W, generator=g) * 4 - 2
        pew = torch.rand(S, 3 * W, generator=g) * 2 - 1
        ew.view(V, 3 * h, 32)[:, :, HD:] = 0                        # heads padded to 32 columns
        pew.view(S, 3 * h, 32)[:, :, HD:] = 0
        ids = torch.randint(1, V, (n_seq, S), generator=g, dtype=torch.int32)
        lens = torch.randint(0, S + 1, (n_seq,), generator=g)
        ids[torch.arange(S)[None, :] >= lens[:, None]] = 0          # padding tails (some sequences all padding)
        ids[0, 0], ids[1, 0] = V - 1, 0
        assert int(ids.max()) == V - 1 and int(ids.min()) == 0
        ew, pew, ids = ew.cuda(), pew.cuda(), ids.cuda().reshape(-1)
        rows = ew[ids.long()] + pew.repeat(n_seq, 1)                # torch fp32: the same single rounding
        scale = 1.0 / math.sqrt(HD)
        want = ops.token_attention(rows[:, :W], rows[:, W:2 * W], rows[:, 2 * W:], n_seq, S, h, HD, scale, head_stride=32)
        torch.cuda.synchronize()
        _CASES[(S, n_seq, h)] = (ew, pew, ids, want, scale)
    return _CASES[(S, n_seq, h)]


@pytest.mark.parametrize('count', ['all', 'minus3', 'zero'])
@pytest.mark.parametrize('S,n_seq,h', SHAPES)
def test_vocab_attention_equals_the_dense_kernel_bitwise(split_forced, S, n_seq, h, count):
    ew, pew, ids, want, scale = _case(S, n_seq, h)
    n_live = {'all': n_seq, 'minus3': n_seq - 3, 'zero': 0}[count]
    n_dev = torch.tensor([n_live], dtype=torch.int32, device='cuda')
    out = torch.full((n_seq * S, h * HD), float('nan'), device='cuda')
    got = ops.token_attention_vocab(ew, pew, ids, n_dev, n_seq, S, h, HD, scale, out=out)
    torch.cuda.synchronize()
    assert got is out
    assert torch.equal(got[:n_live * S], want[:n_live * S])
    assert bool(torch.isnan(got[n_live * S:]).all())                # sequences beyond the device count: untouched


def test_vocab_attention_reports_not_applicable(split_forced):
    ew, pew, ids, want, scale = _case(32, 207, 10)
    assert ops.token_attention_vocab(ew, pew.repeat(3, 1), ids, None, 69, 96, 10, HD, scale) is None      # S outside {32, 64, 128}
    ops.set_split_gemm(False)
    assert ops.token_attention_vocab(ew, pew, ids, None, 207, 32, 10, HD, scale) is None         # the split product switched off
    ops.set_split_gemm(True, force=True)
    assert torch.equal(ops.token_attention_vocab(ew, pew, ids, None, 207, 32, 10, HD, scale), want)   # no device count: every sequence


# ---- the model --------------------------------------------------------------------------------------------------------------------

def _batch(cfg, mode, seed=24):
    batch = synth.make_batch(cfg, 32, 5, seed=seed)
    keys = ('user_title_text', 'user_content_text', 'news_title_text', 'news_content_text')
    if mode == 'no_padding':
        rng = np.random.default_rng(0)
        for k in keys:
            batch[k] = torch.from_numpy(rng.integers(1, cfg.vocabulary_size, size=tuple(batch[k].shape)).astype(np.int32))
    if mode == 'only_padding':
        for k in keys:
            batch[k] = torch.zeros_like(batch[k])
    return batch


def _products(model):
    return model.news_encoder.base_news_encoder._products


def _buffer_ptrs(model):
    wp = _products(model)
    return [t.data_ptr() for e in wp.encoder for t in [e['ew'], e['pew']] + [p for pack in e['ffn'] for p in pack]]


def _switch_off_eager(model, batch, monkeypatch):
    """The same model through the in-graph in_proj, without touching its captured graphs."""
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', False)
    model.use_graph = False
    try:
        return run(model, batch, False)
    finally:
        model.use_graph = True
        monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', True)


@pytest.mark.parametrize('mode', ['mind_shaped', 'no_padding', 'only_padding'])
def test_model_with_and_without_vocab_products(mode, monkeypatch):
    """Config-2 shape.  Both sides carry fp32-level q / k / v and differ only in where one rounding falls: the bound is the one
    tests/test_compact_gpu.py sets between the compacted and the dense path."""
    cfg = make_config(vocabulary_size=3000)
    model, sd = gpu_model(cfg, seed=23)
    batch = _batch(cfg, mode)
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', True)
    got = run(model, batch, False)
    assert _products(model) is not None and all('ew' in e for e in _products(model).encoder)
    # one eager forward under the per-launch profile: no launch gathers word rows -- the path did not fall back
    prof = []
    monkeypatch.setattr(ops, 'PROFILE', prof)
    eager = run(model, batch, False)
    monkeypatch.setattr(ops, 'PROFILE', None)
    assert len(prof) > 10 and all(len(rec) < 8 or rec[7] == 0 for rec in prof)
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', False)
    model._graphs.clear()
    off = run(model, batch, False)
    model._graphs.clear()
    e, e_eager = rel_err(got.numpy(), off.numpy()), rel_err(eager.numpy(), off.numpy())
    print('%s: products vs in_proj %.2e (eager %.2e)' % (mode, e, e_eager))
    assert torch.isfinite(got).all() and e < 2e-6 and e_eager < 2e-6
    if mode == 'mind_shaped':
        want = O.model_forward(sd, cfg, batch)
        e_oracle = rel_err(got.numpy(), want.numpy())
        print('%s: products vs oracle %.2e' % (mode, e_oracle))
        assert e_oracle < 1e-3


def test_stale_products_are_recomputed_in_place_under_the_captured_graph(monkeypatch):
    cfg = make_config(vocabulary_size=3000)
    model, _ = gpu_model(cfg, seed=23)
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', True)
    model.eval()
    ts = TrainStep(model, lr=1e-3, gradient_clip_norm=4.0)         # (re-points the parameters and drops the graphs: before the first capture)
    batch = _batch(cfg, 'mind_shaped')
    enc = model.news_encoder.base_news_encoder
    w = enc.body_transformer.layers[0].self_attn.in_proj_weight
    last = run(model, batch, False)
    ptrs, refreshes = _buffer_ptrs(model), _products(model).refreshes
    assert len(model._graphs) == 1
    graph = next(iter(model._graphs.values()))[0]

    def check(what):
        nonlocal last, refreshes
        got = run(model, batch, False)
        want = _switch_off_eager(model, batch, monkeypatch)
        e = rel_err(got.numpy(), want.numpy())
        print('%s: replay vs switch-off forward %.2e, moved %.2e' % (what, e, rel_err(got.numpy(), last.numpy())))
        assert e < 2e-6, what
        assert not torch.equal(got, last) and rel_err(got.numpy(), last.numpy()) > 1e-4, what
        assert len(model._graphs) == 1 and next(iter(model._graphs.values()))[0] is graph and _buffer_ptrs(model) == ptrs, what
        assert _products(model).refreshes == refreshes + 1, what
        last, refreshes = got, _products(model).refreshes

    with torch.no_grad():
        w.mul_(1.5)                                                # an in-place op: the version counter moves
    check('in-place op')
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for k in sd:                                                   # (the user encoder's view of the news encoder repeats the key)
        if k.endswith('base_news_encoder.word_embedding.weight'):
            sd[k] = sd[k] * 1.25
    model.load_state_dict(sd)
    check('load_state_dict')
    train = [v.cuda() for v in synth.make_batch(cfg, 4, 3, seed=5).values()]
    model.train()
    for _ in range(3):
        ts.step(*train)                                            # the native Adam writes the flat bucket through its address
    model.eval()
    check('TrainStep.step')
    w.data.add_(0.05)                                              # moves neither version nor address ...
    model.weights_changed()                                        # ... so the caller says so
    check('.data edit + weights_changed')
    again = run(model, batch, False)                               # nothing changed: nothing recomputed
    assert torch.equal(again, last) and _products(model).refreshes == refreshes


@pytest.mark.parametrize('how', ['budget', 'switch'])
def test_fall_backs_are_the_in_graph_in_proj_bitwise(how, monkeypatch):
    cfg = make_config(vocabulary_size=3000)
    model, _ = gpu_model(cfg, seed=23)
    batch = _batch(cfg, 'mind_shaped')
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', False)
    want = run(model, batch, False)
    model._graphs.clear()
    enc = model.news_encoder.base_news_encoder
    if how == 'budget':
        monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', True)
        monkeypatch.setattr(enc, 'vocab_qkv_budget', 1)
    got = run(model, batch, False)
    assert torch.equal(got, want)
    wp = getattr(enc, '_products', None)
    assert wp is None if how == 'switch' else all('ew' not in e for e in wp.encoder)
    if how == 'budget':                                            # the budget lifted: the products are built, the graphs dropped
        monkeypatch.setattr(enc, 'vocab_qkv_budget', 1 << 30)
        on = run(model, batch, False)
        assert all('ew' in e for e in enc._products.encoder) and len(model._graphs) == 1
        assert rel_err(on.numpy(), want.numpy()) < 2e-6


def _on_and_off(model, batch, monkeypatch):
    """Logits with the products and, from fresh captures, without; also the per-launch profile of one eager forward with them."""
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', True)
    got = run(model, batch, False)
    prof = []
    monkeypatch.setattr(ops, 'PROFILE', prof)
    run(model, batch, False)
    monkeypatch.setattr(ops, 'PROFILE', None)
    monkeypatch.setattr(newsEncoders, 'VOCAB_QKV', False)
    model._graphs.clear()
    off = run(model, batch, False)
    model._graphs.clear()
    return got, off, prof


def test_chunked_call_site_takes_the_products(monkeypatch):
    """The second call site of CROWN.encode_flat: more news than one pass holds, every chunk on ``encode_tokens_compact``."""
    cfg = make_config(vocabulary_size=3000)
    model, _ = gpu_model(cfg, seed=23)
    batch = _batch(cfg, 'mind_shaped')
    monkeypatch.setattr(newsEncoders, 'MAX_TOKENS_PER_PASS', 32768)            # 1024 titles / 256 bodies per pass of the 1760 news
    enc = model.news_encoder.base_news_encoder
    flat = lambda k, S: torch.cat([batch['news_' + k].reshape(-1, S), batch['user_' + k].reshape(-1, S)]).to(torch.int32).cuda()
    assert not enc._one_pass(flat('title_text', cfg.max_title_length), flat('content_text', cfg.max_abstract_length))
    got, off, prof = _on_and_off(model, batch, monkeypatch)
    e = rel_err(got.numpy(), off.numpy())
    print('chunked: products vs in_proj %.2e' % e)
    assert all('ew' in ent for ent in _products(model).encoder)
    assert len(prof) > 20 and all(len(rec) < 8 or rec[7] == 0 for rec in prof)         # no chunk gathered word rows: none fell back
    assert torch.isfinite(got).all() and e < 2e-6


def test_one_applicable_encoder(monkeypatch):
    """256-token bodies are outside the kernel (S in {32, 64, 128}): the title takes its products, the body keeps its in_proj."""
    cfg = make_config(vocabulary_size=3000, max_abstract_length=256)
    model, _ = gpu_model(cfg, seed=23)
    batch = _batch(cfg, 'mind_shaped')
    got, off, prof = _on_and_off(model, batch, monkeypatch)
    title, body = _products(model).encoder
    assert 'ew' in title and 'ew' not in body and body['ffn'][0] is not None
    gathered = [rec for rec in prof if len(rec) > 7 and rec[7] > 0]
    assert len(gathered) == 2                                                    # the body's in_proj and its padding rows, nothing of the title
    e = rel_err(got.numpy(), off.numpy())
    print('title only: products vs in_proj %.2e' % e)
    assert torch.isfinite(got).all() and e < 2e-6
