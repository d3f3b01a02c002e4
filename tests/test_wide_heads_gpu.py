"""Attention heads wider than 32 columns (csrc/token_attn_wide_f32.hip: 32 < head_dim <= 128, head_dim % 4 == 0, S <= 512) on the GPU:
the kernels against torch CPU statements, the encoder layer with dropout against torch on the kernels' own masks, and the models of
tests/wide_head_cases.py (head_num 3 / 5, MHSA with head_dim 64 / 48) against the reference's goldens and the oracle.

Bounds: the forward keeps test_kernels_gpu.py's TIGHT = 2e-5 against torch's fp32 CPU evaluation (torch fp32 itself is 5e-7 .. 2.7e-6
from fp64 on these shapes), the backward the 2e-4 of test_backward_gpu.py against fp64 autograd (torch fp32: 9e-7 .. 4.5e-6), everything
at model level the 1e-3 of the other model tests."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import wide_head_cases
from dropout_cases import attn_ref          # the attention statement (shared with tests/test_dropout_kernels_gpu.py)
from helpers import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3          # model level, as test_model_gpu.py / test_training_gpu.py / test_fullsize_gpu.py
TIGHT = 2e-5        # test_kernels_gpu.py: exact-fp32 kernels against an fp32 CPU evaluation
BWD = 2e-4          # test_backward_gpu.py: gradients against fp64 autograd


@pytest.fixture(scope='module')
def ops():
    assert torch.cuda.is_available(), 'these tests need the GPU'
    from lime_cikm25_amd import ops as _ops
    from lime_cikm25_amd import _lib
    _lib.load()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def close(got, want, tol, what=''):
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    e = rel_err(got.numpy(), want.detach().numpy())
    print('%s: rel err %.3e (bound %.1e)' % (what, e, tol))
    assert e <= tol, '%s: rel err %.3e > %.1e' % (what, e, tol)
    return e


def packed(vals, hs, fill=0.0):
    """[tok, 3, h, hd] -> the packed qkv buffer [tok, 3 * h * hs] with `fill` in the pad columns."""
    tok, _, h, hd = vals.shape
    buf = torch.full((tok, 3, h, hs), fill)
    buf[..., :hd] = vals
    return buf.view(tok, 3 * h * hs).cuda()


# ---------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------
FWD_SHAPES = [(3, 1, 3, 100, 100), (3, 8, 3, 100, 100), (2, 33, 5, 60, 64), (5, 64, 2, 128, 128), (2, 100, 3, 36, 36), (2, 128, 5, 60, 60),
              (2, 160, 3, 100, 100), (1, 512, 3, 100, 100)]


@pytest.mark.parametrize('n_seq,S,h,hd,hs', FWD_SHAPES)
def test_forward(ops, n_seq, S, h, hd, hs):
    """Plain, lse-writing and device-counted forward; NaN in the pad columns of the hs > hd case (they must never be read)."""
    tok, W, scale = n_seq * S, h * hs, 1.0 / math.sqrt(hd)
    vals = rnd(tok, 3, h, hd, seed=S + hd, scale=2.0)
    want, want_lse = attn_ref(vals, n_seq, S, h, hd, scale)
    g = packed(vals, hs, fill=float('nan'))
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    close(ops.token_attention(q, k, v, n_seq, S, h, hd, scale, head_stride=hs), want, TIGHT, 'forward')
    lse = torch.empty(tok * h, device='cuda')
    close(ops.token_attention(q, k, v, n_seq, S, h, hd, scale, head_stride=hs, lse=lse), want, TIGHT, 'forward with lse')
    close(lse.view(n_seq, S, h).permute(0, 2, 1), want_lse, 1e-5, 'lse')
    # a device-side count below n_seq: the rows of the sequences behind it stay untouched
    live = n_seq - 1
    out = torch.full((tok, h * hd), -7.0, device='cuda')
    ops.token_attention(q, k, v, n_seq, S, h, hd, scale, head_stride=hs, out=out, n_seq_dev=torch.tensor([live], dtype=torch.int32, device='cuda'))
    if live:
        close(out[:live * S], want[:live * S], TIGHT, 'counted forward')
    assert (out[live * S:] == -7.0).all()


def test_forward_key_mask(ops):
    n_seq, S, h, hd = 6, 50, 5, 64
    scale = 1.0 / math.sqrt(hd)
    vals = rnd(n_seq * S, 3, h, hd, seed=51, scale=2.0)
    lens = torch.tensor([1, S, S // 2, 3, S - 1, 0])          # a fully masked row softmaxes to uniform, as in the reference
    mask = torch.arange(S)[None, :] < lens[:, None]
    g, W = packed(vals, hd), h * hd
    got = ops.token_attention(g[:, :W], g[:, W:2 * W], g[:, 2 * W:], n_seq, S, h, hd, scale, key_mask=mask.cuda())
    close(got, attn_ref(vals, n_seq, S, h, hd, scale, mask)[0], TIGHT, 'masked forward')


# ---------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------
def _bwd_ref(vals, dout, n_seq, S, h, hd, scale, mask=None):
    x = vals.double().requires_grad_()
    o, _ = attn_ref(x, n_seq, S, h, hd, scale, mask)
    o.backward(dout.double())
    return o.detach().float(), x.grad.float().reshape(n_seq * S, 3 * h * hd)


@pytest.mark.parametrize('n_seq,S,h,hd', [(2, 16, 3, 100), (2, 50, 5, 60), (1, 128, 2, 128), (2, 200, 3, 100), (1, 512, 3, 100)])
def test_backward(ops, n_seq, S, h, hd):
    tok, W, scale = n_seq * S, h * hd, 1.0 / math.sqrt(hd)
    vals, dout = rnd(tok, 3, h, hd, seed=1), rnd(tok, W, seed=2)
    o, want = _bwd_ref(vals, dout, n_seq, S, h, hd, scale)
    g = packed(vals, hd)
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    dqkv = ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale)
    close(dqkv, want, BWD, 'dqkv')
    again = ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale)
    assert torch.equal(dqkv, again), 'two runs of the backward differ'
    if S > 128:                                                       # the pair the training path uses: out and lse from the forward
        lse = torch.empty(tok * h, device='cuda')
        out = ops.token_attention(q, k, v, n_seq, S, h, hd, scale, lse=lse)
        close(out, o, TIGHT, 'forward')
        close(ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale, out=out, lse=lse), want, BWD,
              'dqkv with the forward statistics')
        close(ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale, out=out), want, BWD, 'dqkv with the forward output')


def test_backward_pad_columns_are_zeros(ops):
    n_seq, S, h, hd, hs = 2, 33, 5, 60, 64
    tok, scale = n_seq * S, 1.0 / math.sqrt(hd)
    vals, dout = rnd(tok, 3, h, hd, seed=3), rnd(tok, h * hd, seed=4)
    _, want = _bwd_ref(vals, dout, n_seq, S, h, hd, scale)
    g, W = packed(vals, hs, fill=float('nan')), h * hs
    dqkv = ops.token_attention_bwd(g[:, :W], g[:, W:2 * W], g[:, 2 * W:], dout.cuda(), n_seq, S, h, hd, scale, head_stride=hs)
    dqkv = dqkv.view(tok, 3, h, hs)
    close(dqkv[..., :hd].reshape(tok, 3 * h * hd), want, BWD, 'dqkv, padded heads')
    assert (dqkv[..., hd:] == 0).all(), 'pad columns must be exact zeros'


def test_backward_key_mask(ops):
    n_seq, S, h, hd = 3, 50, 5, 64
    tok, W, scale = n_seq * S, h * hd, 1.0 / math.sqrt(hd)
    vals, dout = rnd(tok, 3, h, hd, seed=5), rnd(tok, W, seed=6)
    mask = torch.arange(S)[None, :] < torch.tensor([0, S, 17])[:, None]       # sequence 0: every key masked
    o, want = _bwd_ref(vals, dout, n_seq, S, h, hd, scale, mask)
    g = packed(vals, hd)
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    close(ops.token_attention(q, k, v, n_seq, S, h, hd, scale, key_mask=mask.cuda()), o, TIGHT, 'masked forward')
    dqkv = ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale, key_mask=mask.cuda())
    close(dqkv, want, BWD, 'masked dqkv')
    assert torch.equal(dqkv, ops.token_attention_bwd(q, k, v, dout.cuda(), n_seq, S, h, hd, scale, key_mask=mask.cuda()))


# ---------------------------------------------------------------------------------------------------
# the encoder layer with dropout: test_dropout_gpu.py's statement with three heads of 100 columns
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,S', [(3, 16), (2, 128), (2, 200)])
def test_encoder_layer_with_dropout_matches_torch_on_the_same_masks(ops, M, S):
    from lime_cikm25_amd import training as T
    E, nh, Fd, V, p, seed = 300, 3, 512, 400, 0.2, 987654321
    hd = E // nh
    tok = M * S
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V, (M, S), generator=g, dtype=torch.int32)
    names = ['table', 'in_w', 'in_b', 'out_w', 'out_b', 'l1_w', 'l1_b', 'l2_w', 'l2_b', 'n1_w', 'n1_b', 'n2_w', 'n2_b']
    shapes = [(V, E), (3 * E, E), (3 * E,), (E, E), (E,), (Fd, E), (Fd,), (E, Fd), (E,), (E,), (E,), (E,), (E,)]
    vals = {}
    for i, (n, sh) in enumerate(zip(names, shapes)):
        v = rnd(*sh, seed=20 + i, scale=0.5 if n == 'table' else (1.0 / math.sqrt(sh[-1]) if len(sh) == 2 else 0.1))
        if n in ('n1_w', 'n2_w'):
            v = v + 1.0
        vals[n] = v
    pe = rnd(S, E, seed=40)
    G = rnd(M, E, seed=41)

    dev = {n: v.clone().cuda().requires_grad_(True) for n, v in vals.items()}
    pooled = T._TokenEncoder.apply(ids.cuda(), nh, 1e-5, 1e-5, p, seed, dev['table'], pe.cuda(), *[dev[n] for n in names[1:]])
    (pooled * G.cuda()).sum().backward()

    # the kernels' masks, read back through the same generator
    ones = lambda r, c: torch.ones(r, c, device='cuda')
    m_emb = ops.dropout(ones(tok, E), p, seed, T._SITE_EMB).cpu().double()
    m_pe = ops.dropout(ones(tok, E), p, seed, T._SITE_PE).cpu().double()
    m_att = ops.dropout(ones(M * nh * S, S), p, seed, T._SITE_ATTN).cpu().double().view(M, nh, S, S)
    m_d1 = ops.dropout(ones(tok, E), p, seed, T._SITE_DROP1).cpu().double()
    m_ff = ops.dropout(ones(tok, Fd), p, seed, T._SITE_FF).cpu().double()
    m_d2 = ops.dropout(ones(tok, E), p, seed, T._SITE_DROP2).cpu().double()

    # torch fp64 statement of nn.TransformerEncoderLayer (post-LN, ReLU) + the two input dropouts + mean pooling
    ref = {n: v.double().requires_grad_(True) for n, v in vals.items()}
    x0 = m_pe * (m_emb * ref['table'][ids.long().reshape(-1)] + pe.double().repeat(M, 1))
    qkv = x0 @ ref['in_w'].t() + ref['in_b']
    q, k, v = (t.reshape(M, S, nh, hd).permute(0, 2, 1, 3) for t in qkv.split(E, dim=1))
    P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1) * m_att
    ao = (P @ v).permute(0, 2, 1, 3).reshape(tok, E)
    x1 = F.layer_norm(x0 + m_d1 * (ao @ ref['out_w'].t() + ref['out_b']), (E,), ref['n1_w'], ref['n1_b'], 1e-5)
    h = m_ff * torch.relu(x1 @ ref['l1_w'].t() + ref['l1_b'])
    y = F.layer_norm(x1 + m_d2 * (h @ ref['l2_w'].t() + ref['l2_b']), (E,), ref['n2_w'], ref['n2_b'], 1e-5)
    want = y.view(M, S, E).mean(dim=1)
    (want * G.double()).sum().backward()

    assert rel_err(pooled.detach().cpu().numpy(), want.detach().numpy()) < TOL
    worst = ('', 0.0)
    for n in names:
        got, exp = dev[n].grad.cpu().double(), ref[n].grad
        floor = max(float(exp.norm()) / max(1.0, exp.numel()) ** 0.5, 1e-6)
        e = rel_err(got.numpy(), exp.numpy(), floor=floor)
        worst = max(worst, (n, e), key=lambda t: t[1])
        assert e < TOL, '%s: %.3e' % (n, e)
    print('M=%d S=%d: worst gradient %s rel err %.2e' % (M, S, *worst))


# ---------------------------------------------------------------------------------------------------
# refusals: before any launch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,hd,hs', [(16, 132, 132), (16, 50, 52), (513, 100, 100)])
def test_shapes_outside_the_limits_are_refused(ops, S, hd, hs):
    from lime_cikm25_amd import _lib
    h, W = 2, 2 * hs
    g = torch.zeros(S, 3 * W, device='cuda')
    q, k, v = g[:, :W], g[:, W:2 * W], g[:, 2 * W:]
    dout = torch.zeros(S, h * hd, device='cuda')
    calls = [lambda: ops.token_attention(q, k, v, 1, S, h, hd, 1.0, head_stride=hs),
             lambda: ops.token_attention(q, k, v, 1, S, h, hd, 1.0, head_stride=hs, lse=torch.empty(S * h, device='cuda')),
             lambda: ops.token_attention_dropout(q, k, v, 1, S, h, hd, 1.0, 0.1, 1, 2, head_stride=hs),
             lambda: ops.token_attention_bwd(q, k, v, dout, 1, S, h, hd, 1.0, head_stride=hs)]
    for call in calls:
        with pytest.raises(_lib.LimeHipError, match='head_dim <= 128, head_dim % 4 == 0'):
            call()
    from lime_cikm25_amd import training as T
    if hs == hd:
        with pytest.raises(NotImplementedError, match='32 < head_dim <= 128'):
            T._layer_forward(None, torch.zeros(S, 2 * hd, device='cuda'), None, 1, S, 2, 1e-5, 1e-5, 0.0, 0,
                             torch.zeros(6 * hd, 2 * hd, device='cuda'), *([None] * 11))


def test_bf16_with_wide_heads_stays_refused():
    from lime_cikm25_amd import Model, make_config, synth
    cfg = make_config(head_num=3, compute_dtype='bf16', vocabulary_size=5000, max_history_num=3, batch_size=2)
    model = Model(cfg)
    model.initialize()
    model = model.cuda()
    batch = synth.make_batch(cfg, 2, 2, seed=1)
    model.eval()
    model.training = True
    with pytest.raises(NotImplementedError), torch.no_grad():
        model(*[v.cuda() for v in batch.values()])


# ---------------------------------------------------------------------------------------------------
# the models of tests/wide_head_cases.py against the reference's goldens and the oracle
# ---------------------------------------------------------------------------------------------------
def gpu_model(cfg, seed=wide_head_cases.WEIGHT_SEED):
    from lime_cikm25_amd import Model, synth
    m = Model(cfg)
    m.initialize()
    synth.fill_state_dict(m, seed)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.cuda(), sd


def run(model, batch, eval_shape=False):
    model.eval()
    if not eval_shape:
        model.training = True          # [B, K] inputs; children stay in eval mode (no dropout)
    with torch.no_grad():
        out = model(*[v.cuda() for v in batch.values()])
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize('name', list(wide_head_cases.CASES))
def test_forward_matches_the_reference(name):
    from oracle import lime_oracle as O
    cfg, batch, c = wide_head_cases.build_case(name)
    g = load_golden(name)
    model, sd = gpu_model(cfg)
    logits = run(model, batch, c['eval_shape'])
    assert logits.shape == g['logits'].shape
    e = rel_err(logits.numpy(), g['logits'])
    print('%s: logits vs reference golden %.2e' % (name, e))
    assert e < TOL
    if cfg.user_encoder == 'CROWN':
        want = O.model_forward(sd, cfg, batch, eval_shape=c['eval_shape'])
        e = rel_err(logits.numpy(), want.numpy())
        print('%s: logits vs oracle %.2e' % (name, e))
        assert e < TOL
    # the sub-module forwards (the reference's own module API) against the golden's representations
    model.eval()
    b = {k: v.cuda() for k, v in batch.items()}
    if c['eval_shape']:
        for k in list(b):
            if k.startswith('news_') or k == 'remaining_lifetime':
                b[k] = b[k].unsqueeze(1)
    ne, ue = model.news_encoder, model.user_encoder
    with torch.no_grad():
        cand = ne(b['news_title_text'], b['news_title_mask'], b['news_title_entity'], b['news_content_text'], b['news_content_mask'],
                  b['news_content_entity'], b['news_category'], b['news_subCategory'], None, b['news_freshness'],
                  b['news_user_topic_lifetime'])
        assert rel_err(cand.cpu().numpy().reshape(g['news_representation'].shape), g['news_representation']) < TOL
        if not c['eval_shape']:
            user = ue(b['user_title_text'], b['user_title_mask'], b['user_title_entity'], b['user_content_text'], b['user_content_mask'],
                      b['user_content_entity'], b['news_category'], b['news_subCategory'], b['user_category'], b['user_subCategory'],
                      b['user_history_mask'], b['user_history_graph'], b['user_history_category_mask'],
                      b['user_history_category_indices'], None, cand, b['user_freshness'], b['user_user_topic_lifetime'])
            assert tuple(user.shape) == g['user_representation'].shape
            assert rel_err(user.cpu().numpy(), g['user_representation']) < TOL


@pytest.mark.parametrize('name', wide_head_cases.GRAD_CASES)
def test_gradients_match_the_reference(name):
    """Loss and every gradient the reference has within TOL by ``compare_grads``; every parameter it leaves at None has none."""
    from test_naml_gpu import compare_grads, unique_named_parameters
    from lime_cikm25_amd.training import negative_log_softmax
    g = load_golden('grad_' + name)
    cfg, batch, c = wide_head_cases.build_case(name)
    model, _ = gpu_model(cfg)
    model.eval()
    model.training = True
    logits = model(*[v.cuda() for v in batch.values()])
    assert logits.requires_grad
    assert rel_err(logits.detach().cpu().numpy(), g['logits']) < TOL
    loss = negative_log_softmax(logits)
    assert abs(float(loss.detach()) - float(g['loss'])) < TOL * max(1.0, abs(float(g['loss'])))
    loss.backward()
    named = dict(unique_named_parameters(model))
    for k in json.loads(str(g['without_grad'])):
        assert named[k].grad is None, '%s: the reference leaves this gradient at None' % k
    worst = compare_grads(g, named)
    print('%s: loss %.6f (reference %.6f), worst gradient %s rel err %.2e' % (name, float(loss.detach()), float(g['loss']), *worst))


def test_training_step_is_bitwise_reproducible():
    from lime_cikm25_amd.training import TrainStep
    cfg, batch, c = wide_head_cases.build_case('wide_h3')
    b = [v.cuda() for v in batch.values()]

    def train():
        torch.manual_seed(0)
        model = gpu_model(cfg)[0].train()
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        loss = float(TrainStep(model, lr=1e-5, gradient_clip_norm=4.0).step(*b))
        return loss, before, {k: v.detach().clone() for k, v in model.state_dict().items()}

    l1, s0, s1 = train()
    l2, _, s2 = train()
    assert math.isfinite(l1) and l1 == l2
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
    key = 'news_encoder.base_news_encoder.title_transformer.layers.0.self_attn.in_proj_weight'
    assert not torch.equal(s0[key], s1[key])                      # the step did reach the attention's weights


def test_graph_replay_equals_eager_bitwise():
    cfg, batch, c = wide_head_cases.build_case('wide_h3')
    model, _ = gpu_model(cfg)
    model.use_graph = True
    model._graphs.clear()
    first, second = run(model, batch), run(model, batch)
    assert len(model._graphs) == 1
    model.use_graph = False
    want = run(model, batch)
    assert torch.isfinite(want).all() and torch.equal(first, want) and torch.equal(second, want)


def test_news_cache_agrees_with_the_plain_forward(tmp_path):
    """util.compute_scores_cached (Model.build_news_cache + Model.score_behaviors) against util.compute_scores on the toy corpus at
    head_num = 3: the same rank file and metrics, as the cache tests of test_model_gpu.py / test_user_encoders_gpu.py compare them."""
    import os
    from helpers import GOLDEN_DIR
    from lime_cikm25_amd import Model, formats, make_config, util
    from lime_cikm25_amd.device_data import DeviceBehaviors, DeviceCorpus
    g = json.load(open(os.path.join(GOLDEN_DIR, 'formats.json')))
    L = g['lines']
    cfg = make_config(head_num=3, max_history_num=g['max_history_num'], max_title_length=g['max_title_length'],
                      max_abstract_length=g['max_abstract_length'], vocabulary_size=len(g['word_dict']), negative_sample_num=2,
                      category_num=len(g['category_dict']) + 1, subCategory_num=len(g['subCategory_dict']) + 1,
                      user_num=len(g['user_ID_dict']), batch_size=16)
    corpus = formats.build_corpus(cfg, [L['train_news'], L['dev_news'], L['test_news']],
                                  [L['train_behaviors'], L['dev_behaviors'], L['test_behaviors']], g['news_ID_dict'],
                                  g['user_ID_dict'], g['category_dict'], g['subCategory_dict'], g['word_dict'], dataset='adressa')
    dev = DeviceBehaviors.from_devtest(DeviceCorpus(corpus), corpus, 'dev')
    torch.manual_seed(0)
    model = Model(cfg)
    model.initialize()
    torch.nn.init.normal_(model.news_encoder.base_news_encoder.word_embedding.weight, std=0.1)
    torch.nn.init.normal_(model.user_encoder.user_node_embedding, std=0.1)          # zeros at initialisation: make the node term count
    model = model.cuda()
    truth = tmp_path / 'truth.txt'
    with open(truth, 'w') as f:
        for i, labels in enumerate(formats.truth_labels(L['dev_behaviors'])):
            f.write('%d %s\n' % (i + 1, json.dumps(labels).replace(' ', '')))
    a = util.compute_scores(model, [dev.assemble(list(range(dev.num)))], corpus.dev_indices, str(tmp_path / 'rank.txt'), str(truth))
    b = util.compute_scores_cached(model, dev, corpus.dev_indices, str(tmp_path / 'rank_cached.txt'), str(truth), rows_per_forward=dev.num)
    assert open(tmp_path / 'rank_cached.txt').read() == open(tmp_path / 'rank.txt').read()
    assert a == b


def test_default_lengths_against_the_oracle():
    """One scoring forward at the default lengths (batch 8, history 50, title 32, body 128, vocabulary 50000) with head_num = 3."""
    from oracle import lime_oracle as O
    from lime_cikm25_amd import make_config, synth
    cfg = make_config(head_num=3, vocabulary_size=50000, batch_size=8)
    model, sd = gpu_model(cfg, seed=61)
    batch = synth.make_batch(cfg, 8, 5, seed=62)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    want = O.model_forward(sd, cfg, batch)
    got = run(model, batch)
    e = rel_err(got.numpy(), want.numpy())
    print('head_num 3 at the default lengths (B=8): max rel err vs oracle %.2e' % e)
    assert got.shape == (8, 5) and e < TOL
    assert torch.equal(run(model, batch), got)
